"""The device GIF encoder on the CPU: what the numpy restatement (tests/_gif_numpy.py, normative for the kernels of
csrc/gif.hip) is worth.  Pillow opens its files and every frame decodes to palette[indices] exactly over the grid of tests/_gif_cases.py;
the quantiser keeps its invariants; its error is held against Pillow's own quantiser (the route of --gif_encoder pillow) and its stream's
size against Pillow's LZW; the container written by ccedit_amd.gif.write_gif is the restatement's; header, exports and binding agree and
arguments are refused before any HIP call."""
import io
import os

import numpy as np
import pytest
from PIL import Image

import _gif_cases as K
import _gif_numpy as R
from ccedit_amd import gif as G

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _mse(a, b):
    return float(((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean())


def _pillow_quantised(frame):
    """The parent's route: Pillow's adaptive palette (median cut), which does not dither."""
    return np.array(Image.fromarray(frame).quantize(256, dither=Image.Dither.NONE).convert("RGB"))


# ---- the grid and the constants
def test_grid_is_the_issue_grid():
    names = K.names()
    assert len(names) == len(set(names)) == 8 * 9 - 2 + 4            # cells256 / cells257 need 257 pixels: not at 1 x 1; 17 x 19 holds them
    chunks = {f"{h}x{w}": G.chunks_of(h, w) for h, w in K.SIZES}
    assert chunks == {"1x1": 1, "17x19": 1, "33x50": 1, "32x96": 1, "7x439": 2, "48x65": 2, "64x96": 2, "128x192": 8}
    assert 32 * 96 == G.CHUNK and 7 * 439 == G.CHUNK + 1 and 48 * 65 == G.CHUNK + 48 and G.chunks_of(512, 768) == 128
    assert [K.frames(n).shape[0] for n in ("clip2-48x65", "clip5-33x50", "clip5-64x96", "clip2-512x768")] == [2, 5, 5, 2]
    assert (G.FIRST_CODE + G.CHUNK < 4096) and G.SLOT_BYTES * 8 >= 12 * (G.CHUNK + 2) and G.SLOT_BYTES % 16 == 0
    assert G.MOMENT_WORDS * 8 == 5 * 33 ** 3 * 8


def test_contents_are_what_their_names_say():
    occupied = lambda f: len({tuple(c) for c in (f.reshape(-1, 3) >> 3).tolist()})
    assert occupied(K.content("cells256", 48, 65, 1)) == 256 and occupied(K.content("cells257", 48, 65, 1)) == 257
    assert occupied(K.content("colours3", 17, 19, 1)) == 3 and occupied(K.content("colours27", 17, 19, 1)) == 27
    assert occupied(K.content("flat", 7, 439, 1)) == 1 and occupied(K.content("checker", 7, 439, 1)) == 2
    assert (K.content("cells256", 48, 65, 1) & 7).any()              # colours INSIDE their cells, not on the cell grid


# ---- round trip: Pillow decodes the restatement's file to palette[indices]
@pytest.mark.parametrize("name", K.names())
def test_pillow_decodes_the_restatement(name):
    frames = K.frames(name)
    pal, idx = K.reference(name)[:2]
    n, h, w, _ = frames.shape
    data = R.file_bytes(K.encoded(name), G.duration_ms(7), w, h)
    got, info = R.decode_file(io.BytesIO(data))
    assert got.shape == (n, h, w, 3) and info["n_frames"] == n
    assert info["loop"] == 0 and info["duration"] == (G.duration_ms(7) // 10) * 10
    for i in range(n):
        assert np.array_equal(got[i], pal[i][idx[i]]), (name, i)


def test_reference_agrees_with_the_plain_entry_points_of_the_restatement():
    frames = K.frames("clip5-33x50")
    assert R.encode_frames(frames) == K.encoded("clip5-33x50")
    pal, idx = R.quantize(frames)
    assert np.array_equal(pal, K.reference("clip5-33x50")[0]) and np.array_equal(idx, K.reference("clip5-33x50")[1])


@pytest.mark.parametrize("fps", [3, 7, 20])
def test_duration_is_pillows(fps, tmp_path):
    frames = K.frames("clip2-48x65")
    imgs = [Image.fromarray(f) for f in frames]
    theirs = str(tmp_path / "pillow.gif")
    imgs[0].save(theirs, save_all=True, append_images=imgs[1:], duration=int(round(1000.0 / fps)), loop=0)
    ours = G.write_gif(str(tmp_path / "own.gif"), K.encoded("clip2-48x65"), G.duration_ms(fps), 65, 48)
    a, b = Image.open(ours), Image.open(theirs)
    assert a.info["duration"] == b.info["duration"] and a.info["loop"] == b.info["loop"] == 0
    assert a.n_frames == b.n_frames == 2 and a.size == b.size == (65, 48)
    a.seek(1), b.seek(1)
    assert a.info["duration"] == b.info["duration"]


def test_write_gif_writes_the_restatements_file(tmp_path):
    for name in ("1x1-flat", "7x439-noise", "clip5-33x50"):
        n, h, w, _ = K.frames(name).shape
        path = G.write_gif(str(tmp_path / f"{name}.gif"), K.encoded(name), 143, w, h)
        assert open(path, "rb").read() == R.file_bytes(K.encoded(name), 143, w, h)
    with pytest.raises(ValueError, match="no frames"):
        G.write_gif(str(tmp_path / "x.gif"), [], 100, 8, 8)
    with pytest.raises(ValueError, match="H \\* W"):
        G.write_gif(str(tmp_path / "x.gif"), K.encoded("1x1-flat"), 100, 4097, 4096)
    with pytest.raises(ValueError, match="palette"):
        G.write_gif(str(tmp_path / "x.gif"), [(b"\x00" * 767, b"\x00")], 100, 1, 1)
    assert not os.path.exists(str(tmp_path / "x.gif"))


def test_load_video_keyframes_reads_such_a_file(tmp_path):
    from scripts.sampling.util import count_video_frames, load_video_keyframes
    name = "clip5-64x96"
    path = G.write_gif(str(tmp_path / "clip.gif"), K.encoded(name), G.duration_ms(6), 96, 64)
    assert count_video_frames(path) == 5
    kf = load_video_keyframes(path, 6, 3, 3)
    assert tuple(kf.shape) == (3, 3, 64, 96)
    pal, idx = K.reference(name)[:2]
    want = np.stack([pal[i][idx[i]] for i in (0, 2, 4)]).astype(np.float32).transpose(0, 3, 1, 2) / 127.5 - 1.0
    assert np.abs(kf.numpy() - want).max() < 1e-5


# ---- the quantiser's invariants
@pytest.mark.parametrize("name", K.names())
def test_quantiser_invariants(name):
    frames = K.frames(name)
    pal, idx, cells, boxes = K.reference(name)[:4]
    for i, f in enumerate(frames):
        c = (f >> 3).reshape(-1, 3).astype(np.int64)
        k = idx[i].reshape(-1).astype(np.int64)
        b = np.array(boxes[i], np.int64)                            # (K, 6): r0 r1 g0 g1 b0 b1, half open (lo, hi] on the 33 grid = cells lo ... hi - 1
        assert k.max() < len(boxes[i]) <= 256
        for a in range(3):                                          # every pixel's cell lies in its index's box
            assert (c[:, a] >= b[k, 2 * a]).all() and (c[:, a] < b[k, 2 * a + 1]).all()
        vol = (b[:, 1] - b[:, 0]) * (b[:, 3] - b[:, 2]) * (b[:, 5] - b[:, 4])
        assert (vol >= 1).all() and vol.sum() == 32 ** 3              # the boxes tile the grid
        px = f.reshape(-1, 3).astype(np.int64)
        for e in range(256):                                        # palette entries are the rounded box means, unused ones 0
            sel = px[k == e]
            if e < len(boxes[i]):
                assert len(sel) > 0, "a box without pixels was given a palette entry"
                assert pal[i][e].tolist() == ((sel.sum(axis=0) + len(sel) // 2) // len(sel)).tolist()
            else:
                assert len(sel) == 0 and pal[i][e].tolist() == [0, 0, 0]
        occupied = len({tuple(x) for x in c.tolist()})
        if occupied <= 256:                                         # reproduced to within the cell, one entry per occupied cell
            assert len(boxes[i]) == occupied
            assert ((pal[i][idx[i]] >> 3) == (f >> 3)).all()
            if not (f & 7).any() or len({tuple(x) for x in px.tolist()}) == occupied:
                assert np.array_equal(pal[i][idx[i]], f)              # content on the cell grid, or one colour per cell: error 0
        else:
            assert len(boxes[i]) == 256


def test_content_on_the_cell_grid_is_reproduced_exactly():
    rs = np.random.RandomState(3)
    cell = rs.choice(32 ** 3, size=200, replace=False)
    colours = (np.stack([cell >> 10, (cell >> 5) & 31, cell & 31], axis=1) * 8).astype(np.uint8)
    f = colours[rs.randint(0, 200, size=(40, 50))]
    pal, idx, _, boxes = R.quantize_frame(f)
    assert np.array_equal(pal[idx], f) and len(boxes) == len({tuple(x) for x in f.reshape(-1, 3).tolist()})


# ---- quality against the parent's route (Pillow's quantize(256, dither=NONE)), MSE on 8-bit RGB
QUALITY = [("photo", 512, 768, 1.0), ("photo", 64, 96, 1.0), ("noise", 128, 192, 1.0), ("ramp", 256, 384, 1.25), ("ramp", 17, 19, 1.25)]


@pytest.mark.parametrize("content,h,w,factor", QUALITY, ids=[f"{c}-{h}x{w}" for c, h, w, _ in QUALITY])
def test_quality_against_pillows_quantiser(content, h, w, factor):
    """Measured here (seed 3): photo 512 x 768 41.55 against 54.10 (0.768), photo 64 x 96 44.16 against 62.20 (0.710), noise 128 x 192
    162.76 against 439.36 (0.370), ramp 256 x 384 21.50 against 19.92 (1.080), ramp 17 x 19 8.50 against 9.31 (0.913)."""
    f = K.content(content, h, w, seed=3)
    pal, idx, _, _ = R.quantize_frame(f)
    own, theirs = _mse(pal[idx], f), _mse(_pillow_quantised(f), f)
    print(f"{content} {h}x{w}: MSE own {own:.2f}, Pillow {theirs:.2f}, ratio {own / theirs:.3f}")
    assert own <= factor * theirs


def test_flat_and_few_colour_frames_have_no_error():
    for c in ("flat", "colours3", "colours27", "checker"):
        f = K.content(c, 17, 19, seed=2)
        pal, idx, _, _ = R.quantize_frame(f)
        assert np.array_equal(pal[idx], f) and _mse(_pillow_quantised(f), f) == 0.0


# ---- size: the chunk resets cost little
def test_chunked_stream_is_close_to_pillows_lzw():
    """Measured: 491 343 bytes against 491 713 for Pillow's encoding of the same mapped frame (0.999; this photo frame is noisier than a
    decoded sample, both coders spend close to 12 bits per code)."""
    f = K.content("photo", 512, 768, seed=3)
    pal, idx, _, _ = R.quantize_frame(f)
    own = R.file_bytes([(pal.tobytes(), R.lzw_frame(idx))], 100, 768, 512)
    im = Image.fromarray(idx, "P")
    im.putpalette(pal.tobytes())
    b = io.BytesIO()
    im.save(b, "GIF")
    assert np.array_equal(np.array(Image.open(io.BytesIO(b.getvalue())).convert("RGB")), pal[idx])
    print(f"chunked {len(own)} bytes, Pillow {len(b.getvalue())} bytes, ratio {len(own) / len(b.getvalue()):.4f}")
    assert len(own) <= 1.05 * len(b.getvalue())


def test_flat_frame_costs_the_palette_and_the_resets():
    f = K.content("flat", 64, 96, seed=0)
    pal, idx, _, _ = R.quantize_frame(f)
    own = R.file_bytes([(pal.tobytes(), R.lzw_frame(idx))], 100, 96, 64)
    assert len(own) < 768 + 2 * 200 + 100


# ---- LZW: the code widths
@pytest.mark.parametrize("n", K.WIDTH_EDGES + [G.CHUNK])
def test_lzw_width_edges_decode(n):
    """A chunk of n pixels without a repeating pair emits n codes; the width after them is what a decoder that lags one entry expects, as
    the frame's only chunk (EOI) and as the first of two (Clear).  Pillow decodes both files to the input."""
    s = K.pairless_stream(n + 5)
    pal = np.stack([np.arange(256)] * 3, axis=1).astype(np.uint8)
    (bits, length, codes), = R.lzw_chunks(s[:n], chunk=n)
    assert codes == n
    width_end = 9 + (n >= 255) + (n >= 767) + (n >= 1791)
    widths = sum(9 + (k >= 255) + (k >= 767) + (k >= 1791) for k in range(n))          # the code after k earlier ones: next free code 258 + k
    assert length == 9 + widths + width_end
    assert bits >> (length - width_end) == G.EOI and bits & 511 == G.CLEAR
    got, _ = R.decode_file(io.BytesIO(R.file_bytes([(pal.tobytes(), R.lzw_frame(s[:n], chunk=n))], 100, n, 1)))
    assert np.array_equal(got[0, 0, :, 0], s[:n])
    first, second = R.lzw_chunks(s, chunk=n)
    assert first[2] == n and first[1] == length and first[0] >> (length - width_end) == G.CLEAR
    assert second[0] & 511 != G.CLEAR                                   # only the frame's first chunk starts with a Clear
    got, _ = R.decode_file(io.BytesIO(R.file_bytes([(pal.tobytes(), R.lzw_frame(s, chunk=n))], 100, n + 5, 1)))
    assert np.array_equal(got[0, 0, :, 0], s)
    if n == G.CHUNK:
        assert width_end == 12


# ---- the host side of the encoder refuses before any launch
def test_sizes_are_refused_with_a_message():
    for h, w in ((0, 8), (8, 0), (65536, 1), (1, 65536), (4096, 4097)):
        with pytest.raises(ValueError, match="H \\* W <= 2\\^24"):
            G.check_size(h, w)
    G.check_size(4096, 4096), G.check_size(1, 65535), G.check_size(65535, 256)
    import torch
    for bad in (torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 8, 8, 3), np.zeros((1, 8, 8, 3), np.uint8)):
        with pytest.raises(ValueError, match="on the device"):
            G.encode_frames(bad)
        with pytest.raises(ValueError, match="on the device"):
            G.quantize(bad)


def test_frames_per_launch_follows_the_scratch_bound(monkeypatch):
    assert G.frames_per_launch(512, 768) == G.MAX_FRAMES_PER_LAUNCH
    monkeypatch.setattr(G, "SCRATCH_BYTES", 8 << 20)
    assert G.frames_per_launch(512, 768) == 2
    monkeypatch.setattr(G, "SCRATCH_BYTES", 1)
    assert G.frames_per_launch(512, 768) == 1


def test_entry_level_refuses_bad_encoders(tmp_path):
    import torch
    from scripts.sampling import sampling_tv2v as S
    from scripts.sampling.util import perform_save_locally_video, save_gif_u8
    with pytest.raises(ValueError, match="gif_encoder"):
        save_gif_u8(str(tmp_path), np.zeros((1, 8, 8, 3), np.uint8), 3, gif_encoder="gpu")
    with pytest.raises(ValueError, match="savetype must be 'gif'"):
        perform_save_locally_video(str(tmp_path), torch.zeros(1, 3, 2, 8, 8), 3, "npy", gif_encoder="device")
    assert not os.listdir(str(tmp_path))
    p = S.make_parser()
    assert p.parse_args([]).gif_encoder == "pillow"
    for save_type in ("npy", "mjpeg"):
        with pytest.raises(SystemExit):
            S.check_args(p, p.parse_args(["--gif_encoder", "device", "--save_type", save_type]))
    S.check_args(p, p.parse_args(["--gif_encoder", "device", "--save_type", "gif"]))
    S.check_args(p, p.parse_args(["--gif_encoder", "pillow", "--save_type", "npy"]))


def test_pillow_branch_writes_the_same_bytes_as_before(tmp_path):
    """The default is untouched: save_gif_u8 and perform_save_locally_video write what the plain Pillow call writes."""
    import torch
    from scripts.sampling.util import perform_save_locally_video, save_gif_u8
    frames = K.frames("clip5-33x50")
    imgs = [Image.fromarray(f) for f in frames]
    want = io.BytesIO()
    imgs[0].save(want, "GIF", save_all=True, append_images=imgs[1:], duration=int(round(1000.0 / 7)), loop=0)
    assert open(save_gif_u8(str(tmp_path / "a"), frames, 7), "rb").read() == want.getvalue()
    x = torch.from_numpy(frames.astype(np.float32) / 255.0).permute(3, 0, 1, 2)[None]
    u8 = (255.0 * x[0].permute(1, 2, 3, 0).numpy()).astype(np.uint8)
    imgs = [Image.fromarray(f) for f in u8]
    want = io.BytesIO()
    imgs[0].save(want, "GIF", save_all=True, append_images=imgs[1:], duration=int(round(1000.0 / 7)), loop=0)
    p, = perform_save_locally_video(str(tmp_path / "b"), x, 7, "gif", return_savepaths=True, save_grid=False)
    assert open(p, "rb").read() == want.getvalue()


# ---- the C ABI: header, exports and binding agree (the conventions of tests/test_cabi.py)
def test_cabi_gif():
    import ctypes
    import re
    from ccedit_amd import hip
    from ccedit_amd.csrc.build import build
    lib = ctypes.CDLL(build(force=False, verbose=False))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ccedit_hip.h")).read(), flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(ccedit_[a-z0-9_]+)\s*\(", src)) if n.startswith("ccedit_gif_"))
    assert declared == ["ccedit_gif_histogram", "ccedit_gif_lzw", "ccedit_gif_map", "ccedit_gif_pack", "ccedit_gif_pack_scan", "ccedit_gif_palette",
                        "ccedit_gif_slot_bytes"]
    for n in declared:
        assert hasattr(lib, n) and n in hip.EXPORTS
        args = re.search(re.escape(n) + r"\s*\(([^)]*)\)", src).group(1)
        assert len(hip._SIGS[n][1]) == (0 if args.strip() == "void" else len(args.split(","))), n
    assert "#define CCEDIT_ABI_VERSION 12" in src and hip.ABI_VERSION == 12
    l = hip.lib()                                              # argument validation runs before any HIP call
    assert l.ccedit_gif_slot_bytes() == G.SLOT_BYTES == 4624
    assert l.ccedit_gif_histogram(None, 16, 1, 8, 8, None) == -1 and b"null" in l.ccedit_last_error()
    assert l.ccedit_gif_histogram(16, 12, 1, 8, 8, None) == -1 and b"aligned" in l.ccedit_last_error()
    assert l.ccedit_gif_histogram(16, 16, 0, 8, 8, None) == -1 and b"N=0" in l.ccedit_last_error()
    assert l.ccedit_gif_histogram(16, 16, 1, 0, 8, None) == -1 and b"0x8" in l.ccedit_last_error()
    assert l.ccedit_gif_histogram(16, 16, 1, 4096, 4097, None) == -1 and b"2^24" in l.ccedit_last_error()
    assert l.ccedit_gif_histogram(16, 16, 1, 1, 65536, None) == -1
    assert l.ccedit_gif_histogram(16, 16, 600, 4096, 4096, None) == -1 and b"2^33" in l.ccedit_last_error()
    assert l.ccedit_gif_palette(16, None, 16, 1, None) == -1 and b"null" in l.ccedit_last_error()
    assert l.ccedit_gif_palette(16, 16, 16, 0, None) == -1 and b"N=0" in l.ccedit_last_error()
    assert l.ccedit_gif_palette(20, 16, 16, 1, None) == -1 and b"aligned" in l.ccedit_last_error()
    assert l.ccedit_gif_map(16, None, 16, 1, 8, 8, None) == -1 and b"null" in l.ccedit_last_error()
    assert l.ccedit_gif_map(16, 16, 16, 1, 8, 70000, None) == -1
    assert l.ccedit_gif_lzw(16, 16, None, 1, 8, 8, 3072, None) == -1 and b"null" in l.ccedit_last_error()
    assert l.ccedit_gif_lzw(16, 16, 16, 1, 8, 8, 3073, None) == -1 and b"chunk=3073" in l.ccedit_last_error()
    assert l.ccedit_gif_lzw(16, 16, 16, 1, 8, 8, 0, None) == -1 and b"chunk=0" in l.ccedit_last_error()
    assert l.ccedit_gif_lzw(16, 18, 16, 1, 8, 8, 3072, None) == -1 and b"aligned" in l.ccedit_last_error()
    assert l.ccedit_gif_lzw(16, 16, 16, 1, 4096, 4096, 1, None) == -1 and b"2^22 chunks" in l.ccedit_last_error()
    assert l.ccedit_gif_pack_scan(16, 16, None, 1, 8, 8, 3072, None) == -1 and b"null" in l.ccedit_last_error()
    assert l.ccedit_gif_pack_scan(16, 12, 16, 1, 8, 8, 3072, None) == -1 and b"aligned" in l.ccedit_last_error()
    assert l.ccedit_gif_pack_scan(16, 16, 16, 1, 8, 8, 4000, None) == -1 and b"chunk=4000" in l.ccedit_last_error()
    assert l.ccedit_gif_pack(16, 16, 16, None, 1, 8, 8, 3072, 10, None) == -1 and b"null" in l.ccedit_last_error()
    assert l.ccedit_gif_pack(16, 16, 16, 16, 1, 8, 8, 3072, 0, None) == -1 and b"out_bytes=0" in l.ccedit_last_error()
    assert l.ccedit_gif_pack(16, 16, 16, 18, 1, 8, 8, 3072, 10, None) == -1 and b"aligned" in l.ccedit_last_error()
    assert l.ccedit_gif_pack(16, 16, 16, 16, 70000, 8, 8, 3072, 10, None) == -1 and b"N=70000" in l.ccedit_last_error()
