"""GIF output encoded on a real MI355X (ccedit_amd/gif.py, csrc/gif.hip, --gif_encoder device).

Exact (no tolerance anywhere): encode_frames and every stage against the numpy restatement (tests/_gif_numpy.py, whose own worth
tests/test_gif.py checks) over the grid of tests/_gif_cases.py — nine sizes, nine contents, clips of 1, 2 and 5 frames —, the LZW and pack
stages alone on index streams that sit on the code-width edges, independence of the frames-per-launch and scratch bounds, chunk lengths
held in range, argument validation through ops, and the entry level: perform_save_locally_video, save_gif_u8 and one job of
sampling_tv2v.py write files that Pillow decodes to the restatement of the uint8 frames the Pillow branch would have quantised."""
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gif_cases as K  # noqa: E402
import _gif_numpy as R  # noqa: E402
from ccedit_amd import gif as G  # noqa: E402

pytestmark = pytest.mark.gpu

GREY = np.stack([np.arange(256)] * 3, axis=1).astype(np.uint8).tobytes()      # palette under which an index decodes to itself


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _slot_bytes(slots, i, nbits):
    return slots[i, :(nbits + 7) // 8].tobytes()


def _chunk_bytes(bits, nbits):
    return bits.to_bytes((nbits + 7) // 8, "little")


# ---- 1. bit equality, end to end and stage by stage -------------------------------------------------
@pytest.mark.parametrize("name", K.names())
def test_encode_frames_equals_the_restatement(name):
    _need_gpu()
    got = G.encode_frames(_dev(K.frames(name)))
    want = K.encoded(name)
    assert [(len(p), len(s)) for p, s in got] == [(len(p), len(s)) for p, s in want], name
    assert got == want, name
    pal, idx = G.quantize(_dev(K.frames(name)))
    assert np.array_equal(pal.cpu().numpy(), K.reference(name)[0]) and np.array_equal(idx.cpu().numpy(), K.reference(name)[1])


@pytest.mark.parametrize("name", K.names())
def test_stage_outputs(name):
    _need_gpu()
    from ccedit_amd import ops
    frames = K.frames(name)
    n, h, w, _ = frames.shape
    pal, idx, cells, boxes, chunks, streams = K.reference(name)
    d = _dev(frames)
    want_m = np.stack([R.moments(f) for f in frames])
    moments = ops.gif_histogram(d)
    assert moments.dtype == torch.int64 and tuple(moments.shape) == (n, 5, 33, 33, 33)
    assert np.array_equal(moments.cpu().numpy(), want_m)
    assert int(want_m[:, 0].sum()) == n * h * w
    got_cells, got_pal = ops.gif_palette(moments)                     # (the moments become their prefix sums in place)
    assert np.array_equal(moments.cpu().numpy(), np.stack([R.prefix(m) for m in want_m]))
    assert np.array_equal(got_cells.cpu().numpy(), cells)
    assert np.array_equal(got_pal.cpu().numpy(), pal)
    got_idx = ops.gif_map(d, got_cells)
    assert np.array_equal(got_idx.cpu().numpy(), idx)
    slots, chunk_bits = ops.gif_lzw(got_idx)
    c = G.chunks_of(h, w)
    flat = [x for ch in chunks for x in ch]
    assert tuple(slots.shape) == (n * c, G.SLOT_BYTES) and chunk_bits.cpu().tolist() == [x[1] for x in flat]
    s = slots.cpu().numpy()
    for i, (bits, nbits, _) in enumerate(flat):
        assert _slot_bytes(s, i, nbits) == _chunk_bytes(bits, nbits), (name, i)
    chunk_off, frame_bytes = ops.gif_pack_scan(chunk_bits, n, h, w)
    assert frame_bytes.cpu().tolist() == [len(x) for x in streams]
    offs, at = [], 0
    for ch in chunks:
        for _, nbits, _ in ch:
            offs.append(at)
            at += nbits
        at = (at + 7) // 8 * 8
    assert chunk_off.cpu().tolist() == offs
    out = ops.gif_pack(slots, chunk_bits, chunk_off, n, h, w, G.CHUNK, at // 8)
    assert out.cpu().numpy().tobytes() == b"".join(streams)


def test_production_size_file_decodes(tmp_path):
    _need_gpu()
    name = "clip2-512x768"
    path = G.write_gif(str(tmp_path / "big.gif"), G.encode_frames(_dev(K.frames(name))), G.duration_ms(3), 768, 512)
    got, info = R.decode_file(path)
    pal, idx = K.reference(name)[:2]
    assert info["n_frames"] == 2 and info["duration"] == 330
    assert np.array_equal(got, np.stack([pal[i][idx[i]] for i in range(2)]))
    assert np.array_equal(got[1], K.frames(name)[1])                  # the white frame: one box, its mean


# ---- 2. the code-width edges: LZW and pack alone, fed index arrays --------------------------------
def _lzw_and_pack(indices, chunk):
    from ccedit_amd import ops
    n, h, w = indices.shape
    slots, chunk_bits = ops.gif_lzw(_dev(indices), chunk)
    chunk_off, frame_bytes = ops.gif_pack_scan(chunk_bits, n, h, w, chunk)
    sizes = frame_bytes.cpu().tolist()
    packed = ops.gif_pack(slots, chunk_bits, chunk_off, n, h, w, chunk, sum(sizes)).cpu().numpy().tobytes()
    return chunk_bits.cpu().tolist(), sizes, packed


@pytest.mark.parametrize("n", K.WIDTH_EDGES + [G.CHUNK])
def test_code_width_edges(n):
    """A chunk of n pixels in which no pair repeats emits exactly n codes: n = 253 ... 258, 765 ... 770, 1789 ... 1794 walk the next free
    code across 512, 1024 and 2048, n = 3072 takes the width to 12 bits.  As the frame's only chunk (ends with EOI) and as the first of two
    (ends with Clear at the width it finished with).  Both files must also decode in Pillow to the input."""
    _need_gpu()
    s = K.pairless_stream(n + 5)
    for pixels in (n, n + 5):
        idx = s[:pixels].reshape(1, 1, pixels)
        want_chunks = R.lzw_chunks(idx, chunk=n)
        assert want_chunks[0][2] == n and len(want_chunks) == (1 if pixels == n else 2)
        want = R.lzw_frame(idx, chunk=n)
        lens, sizes, packed = _lzw_and_pack(idx, n)
        assert lens == [c[1] for c in want_chunks] and sizes == [len(want)]
        assert packed == want, (n, pixels)
        got, _ = R.decode_file(io.BytesIO(R.file_bytes([(GREY, packed)], 100, pixels, 1)))
        assert np.array_equal(got[0, 0, :, 0], s[:pixels])
    assert G.encode_indices(_dev(s[:n].reshape(1, 1, n)), n) == [R.lzw_frame(s[:n], chunk=n)]


def test_small_chunks_and_several_frames():
    """Chunks far below a byte boundary's period: 7 pixels each, three frames of 50 pixels (eight chunks, the last of one pixel) — every
    chunk starts in the middle of a word of the output, frames start on byte boundaries."""
    _need_gpu()
    rs = np.random.RandomState(4)
    idx = rs.randint(0, 4, size=(3, 5, 10)).astype(np.uint8)
    lens, sizes, packed = _lzw_and_pack(idx, 7)
    want = [R.lzw_frame(f, chunk=7) for f in idx]
    assert lens == [c[1] for f in idx for c in R.lzw_chunks(f, chunk=7)]
    assert sizes == [len(x) for x in want] and packed == b"".join(want)
    for i, x in enumerate(want):
        got, _ = R.decode_file(io.BytesIO(R.file_bytes([(GREY, x)], 100, 10, 5)))
        assert np.array_equal(got[0, :, :, 0], idx[i])


# ---- 3. bounds -------------------------------------------------------------------------------------
def test_result_does_not_depend_on_the_launch_bounds(monkeypatch):
    _need_gpu()
    name = "clip5-64x96"
    d = _dev(K.frames(name))
    want = K.encoded(name)
    assert G.frames_per_launch(64, 96) >= 5 and G.encode_frames(d) == want          # all five in one launch
    for per in (1, 3):
        monkeypatch.setattr(G, "MAX_FRAMES_PER_LAUNCH", per)
        assert G.frames_per_launch(64, 96) == per
        assert G.encode_frames(d) == want, per
        pal, idx = G.quantize(d)
        assert np.array_equal(pal.cpu().numpy(), K.reference(name)[0]) and np.array_equal(idx.cpu().numpy(), K.reference(name)[1])
    monkeypatch.setattr(G, "MAX_FRAMES_PER_LAUNCH", 64)
    per_frame = G.MOMENT_WORDS * 8
    for scratch, per in ((1, 1), (3 * per_frame + 3 * 200000, 3), (1 << 30, 64)):
        monkeypatch.setattr(G, "SCRATCH_BYTES", scratch)
        assert G.frames_per_launch(64, 96) == per
        assert G.encode_frames(d) == want, scratch
    assert [G.encode_frames(d[i:i + 1])[0] for i in range(5)] == want
    for _ in range(3):
        assert G.encode_frames(d) == want                                         # integer atomics: repeats are bit-equal


def test_nothing_around_the_buffers_is_written():
    _need_gpu()
    from ccedit_amd import hip, ops
    name = "clip2-48x65"
    frames = K.frames(name)
    n, h, w, _ = frames.shape
    nbytes = frames.size
    for fill in (0xA5, 0x00):
        big = torch.full((nbytes + 8192,), fill, dtype=torch.uint8, device="cuda")
        big[4096:4096 + nbytes] = _dev(frames).reshape(-1)
        assert G.encode_frames(big[4096:4096 + nbytes].view(n, h, w, 3)) == K.encoded(name)
        assert bool((big[:4096] == fill).all()) and bool((big[4096 + nbytes:] == fill).all())
    idx = _dev(K.reference(name)[1])
    slots, chunk_bits = ops.gif_lzw(idx)
    canary = torch.full_like(slots, 0x5A)
    hip.check(hip.lib().ccedit_gif_lzw(idx.data_ptr(), canary.data_ptr(), chunk_bits.data_ptr(), n, h, w, G.CHUNK,
                                       torch.cuda.current_stream().cuda_stream), "ccedit_gif_lzw")
    c = canary.cpu().numpy()
    for i, nbits in enumerate(chunk_bits.cpu().tolist()):
        assert (c[i, (nbits + 31) // 32 * 4:] == 0x5A).all(), f"chunk {i}: bytes written behind its last word"


def test_chunk_lengths_are_held_in_the_slot():
    """Chunk bit lengths are device data when the pack stages read them: whatever they hold is clamped into 0 ... 8 x slot bytes, the
    offsets follow the clamped values, and the copy stays inside the output."""
    _need_gpu()
    from ccedit_amd import ops
    n, h, w = 2, 64, 96
    c = G.chunks_of(h, w)
    slots = torch.zeros((n * c, G.SLOT_BYTES), dtype=torch.uint8, device="cuda")
    bad = np.array([-5, 2 ** 31 - 1, 100, -2 ** 31], np.int32)
    held = np.clip(bad.astype(np.int64), 0, G.SLOT_BYTES * 8)
    chunk_off, frame_bytes = ops.gif_pack_scan(_dev(bad), n, h, w)
    sizes = [int((held[2 * f] + held[2 * f + 1] + 7) // 8) for f in range(n)]
    assert frame_bytes.cpu().tolist() == sizes
    assert chunk_off.cpu().tolist() == [0, int(held[0]), sizes[0] * 8, sizes[0] * 8 + int(held[2])]
    out = ops.gif_pack(slots, _dev(bad), chunk_off, n, h, w, G.CHUNK, sum(sizes))
    torch.cuda.synchronize()
    assert out.numel() == sum(sizes) and not bool(out.any())
    short = ops.gif_pack(slots, _dev(bad), chunk_off, n, h, w, G.CHUNK, 8)       # an output the offsets do not fit: those chunks are skipped
    torch.cuda.synchronize()
    assert short.numel() == 8


def test_argument_validation():
    _need_gpu()
    from ccedit_amd import ops
    frames = _dev(K.frames("17x19-photo"))
    moments = ops.gif_histogram(frames)
    with pytest.raises(ValueError, match="gif_histogram"):
        ops.gif_histogram(frames.cpu())
    with pytest.raises(ValueError, match="gif_histogram"):
        ops.gif_histogram(frames[..., :2].contiguous())
    with pytest.raises(ValueError, match="gif_histogram"):
        ops.gif_histogram(frames.float())
    with pytest.raises(ValueError, match="H \\* W <= 2\\^24"):
        ops.gif_histogram(torch.zeros((1, 1, 65536, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="moments"):
        ops.gif_palette(moments[:, :4].contiguous())
    with pytest.raises(ValueError, match="moments"):
        ops.gif_palette(moments.int())
    cells, palettes = ops.gif_palette(moments)
    assert tuple(cells.shape) == (1, 32, 32, 32) and tuple(palettes.shape) == (1, 256, 3)
    with pytest.raises(ValueError, match="cells"):
        ops.gif_map(frames, cells[:, :31].contiguous())
    with pytest.raises(ValueError, match="cells"):
        ops.gif_map(frames, torch.cat([cells, cells]))
    idx = ops.gif_map(frames, cells)
    for chunk in (0, G.CHUNK + 1, 2.5):
        with pytest.raises(ValueError, match="chunk"):
            ops.gif_lzw(idx, chunk)
    with pytest.raises(ValueError, match="indices"):
        ops.gif_lzw(idx[0])
    slots, chunk_bits = ops.gif_lzw(idx)
    with pytest.raises(ValueError, match="chunk_bits"):
        ops.gif_pack_scan(chunk_bits, 2, 17, 19)
    with pytest.raises(ValueError, match="chunk_bits"):
        ops.gif_pack_scan(chunk_bits.long(), 1, 17, 19)
    chunk_off, frame_bytes = ops.gif_pack_scan(chunk_bits, 1, 17, 19)
    with pytest.raises(ValueError, match="slots"):
        ops.gif_pack(slots[:, :-1].contiguous(), chunk_bits, chunk_off, 1, 17, 19, G.CHUNK, int(frame_bytes.sum()))
    with pytest.raises(ValueError, match="chunk_off"):
        ops.gif_pack(slots, chunk_bits, chunk_off.int(), 1, 17, 19, G.CHUNK, int(frame_bytes.sum()))
    with pytest.raises(ValueError, match="out_bytes"):
        ops.gif_pack(slots, chunk_bits, chunk_off, 1, 17, 19, G.CHUNK, 0)
    with pytest.raises(ValueError, match="on the device"):
        G.encode_frames(frames.cpu())
    with pytest.raises(ValueError, match="H \\* W <= 2\\^24"):
        G.encode_frames(torch.zeros((1, 65536, 1, 3), dtype=torch.uint8, device="cuda"))
    assert G.encode_frames(frames) == K.encoded("17x19-photo")


# ---- 4. the entry level ----------------------------------------------------------------------------
def _decoded(path):
    return R.decode_file(path)[0]


def _restated(u8):
    pal, idx = R.quantize(u8)
    return np.stack([pal[i][idx[i]] for i in range(len(u8))])


def test_save_functions_number_files_alike_and_both_routes_write_the_same_bytes(tmp_path):
    _need_gpu()
    from scripts.sampling.util import perform_save_locally_video, save_gif_u8
    g = torch.Generator().manual_seed(2)
    x = torch.rand(2, 3, 4, 32, 48, generator=g)
    pil, host, dev = str(tmp_path / "pillow"), str(tmp_path / "host"), str(tmp_path / "dev")
    p_pil = perform_save_locally_video(pil, x, 5, "gif", return_savepaths=True)
    p_pil += perform_save_locally_video(pil, x[:1], 5, "gif", return_savepaths=True, save_grid=False)
    p0 = perform_save_locally_video(host, x, 5, "gif", return_savepaths=True, gif_encoder="device")
    p0 += perform_save_locally_video(host, x[:1], 5, "gif", return_savepaths=True, save_grid=False, gif_encoder="device")
    assert [os.path.relpath(p, host) for p in p0] == [os.path.relpath(p, pil) for p in p_pil] == [os.path.join("gif", f"animation-{i:04}.gif")
                                                                                                  for i in range(3)]
    assert sorted(os.listdir(os.path.join(host, "grid"))) == sorted(os.listdir(os.path.join(pil, "grid"))) == ["grid-0000.png", "grid-0001.png"]
    for nm in ("grid-0000.png", "grid-0001.png"):                   # the grid PNG is untouched
        assert open(os.path.join(host, "grid", nm), "rb").read() == open(os.path.join(pil, "grid", nm), "rb").read()
    p1 = perform_save_locally_video(dev, x.cuda(), 5, "gif", return_savepaths=True, gpu_io=True, gif_encoder="device")
    assert [open(p, "rb").read() for p in p1] == [open(p, "rb").read() for p in p0[:2]], "with and without gpu_io the device encoder differs"
    p2 = perform_save_locally_video(dev, (x * 2 - 1).cuda(), 5, "gif", return_savepaths=True, gpu_io=True, signed=True, save_grid=False,
                                    gif_encoder="device")
    assert [os.path.basename(p) for p in p2] == ["animation-0002.gif", "animation-0003.gif"]
    for b in range(2):
        u8 = (255.0 * x[b].permute(1, 2, 3, 0).numpy()).astype(np.uint8)          # what the Pillow branch would have quantised
        assert np.array_equal(_decoded(p0[b]), _restated(u8))
        assert open(p0[b], "rb").read() == R.file_bytes(R.encode_frames(u8), G.duration_ms(5), 48, 32)
        from PIL import Image
        assert Image.open(p0[b]).info["duration"] == Image.open(p_pil[b]).info["duration"] == 200
    # save_gif_u8: a host array (uploaded once) and a device tensor
    u8 = K.frames("clip5-33x50")
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    assert save_gif_u8(a, u8, 7, gif_encoder="device") == os.path.join(a, "gif", "animation-0000.gif")
    assert save_gif_u8(a, _dev(u8), 7, gif_encoder="device") == os.path.join(a, "gif", "animation-0001.gif")
    assert save_gif_u8(b, u8, 7) == os.path.join(b, "gif", "animation-0000.gif")
    one, two = (open(os.path.join(a, "gif", f"animation-000{i}.gif"), "rb").read() for i in (0, 1))
    assert one == two == R.file_bytes(K.encoded("clip5-33x50"), G.duration_ms(7), 50, 33)
    assert np.array_equal(_decoded(os.path.join(a, "gif", "animation-0000.gif")), _restated(u8))


def _write_config(tmp_path):
    import yaml
    from ccedit_amd.sgm_compat import engine_config
    cfg = os.path.join(str(tmp_path), "tv2v.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump(dict(model=engine_config(crossframe=False, vae_ch=32, model_channels=64, num_heads=2, context_dim=64)), f)
    return cfg


@pytest.mark.timeout(900)
def test_entry_point_writes_device_gifs(tmp_path, monkeypatch):
    """sampling_tv2v.py --synthetic --gpu_io --propagate --save_type gif --gif_encoder device on a frame directory (8 frames, 3 keyframes
    at gap 3, 64 x 128 output): every .gif the job writes — original/, result/, control_hint/ and result_full/ — decodes to the
    restatement of the frames handed to gif.encode_frames, and the set of files is that of a --gif_encoder pillow run."""
    _need_gpu()
    from PIL import Image
    from scripts.sampling import sampling_tv2v as S
    cfg = _write_config(tmp_path)
    vdir = tmp_path / "clips" / "fox"
    vdir.mkdir(parents=True)
    big = K.smoothed(96 + 20, 160 + 40, 30)
    for i in range(8):
        Image.fromarray(big[2 * i:2 * i + 96, 4 * i:4 * i + 160]).save(str(vdir / f"{i:03d}.png"))
    base = ["sampling_tv2v.py", "--config_path", cfg, "--synthetic", "--H", "64", "--W", "128", "--num_keyframes", "3", "--sample_steps", "2",
            "--sampler_name", "DPMPP2SAncestralSampler", "--original_fps", "9", "--target_fps", "3", "--noise_seed", "1", "--prompt", "a red fox",
            "--video_path", str(vdir), "--batch_size", "1", "--save_type", "gif", "--gpu_io", "--propagate"]
    handed, written = [], []
    real_encode, real_write = G.encode_frames, G.write_gif

    def encode(frames):
        assert frames.is_cuda and frames.dtype == torch.uint8, "under --gpu_io the frames stay on the device"
        handed.append(frames.cpu().numpy().copy())
        return real_encode(frames)

    def write(path, *a, **k):
        written.append(path)
        return real_write(path, *a, **k)

    monkeypatch.setattr(G, "encode_frames", encode)
    monkeypatch.setattr(G, "write_gif", write)
    files = {}
    try:
        for tag in ("device", "pillow"):
            out = str(tmp_path / tag)
            monkeypatch.setattr(sys, "argv", base + ["--save_path", out, "--gif_encoder", tag])
            S.main()
            files[tag] = sorted(os.path.relpath(os.path.join(root, nm), out) for root, _, names in os.walk(out) for nm in names)
            if tag == "device":
                log = json.load(open(os.path.join(out, "default", "log_info.json")))
                n_device = len(written)
    finally:
        torch.set_grad_enabled(True)
    assert len(written) == n_device, "the pillow run reached the device encoder"
    assert files["device"] == files["pillow"]
    gifs = [f for f in files["device"] if f.endswith(".gif")]
    out = str(tmp_path / "device")
    assert sorted(os.path.relpath(p, out) for p in written) == gifs and len(gifs) == 4
    assert {os.path.dirname(os.path.relpath(p, os.path.join(out, "default"))) for p in written} == {
        os.path.join(d, "gif") for d in ("original", "result", "control_hint", "result_full")}
    assert log["keyframes_paths"] == [os.path.join(out, "default", "result", "gif", "animation-0000.gif")]
    assert log["fullrate_paths"] == [os.path.join(out, "default", "result_full", "gif", "animation-0000.gif")]
    assert len(handed) == len(written)
    for frames, path in zip(handed, written):
        got, info = R.decode_file(path)
        assert got.shape == frames.shape and frames.shape[1:] == (64, 128, 3)
        assert np.array_equal(got, _restated(frames)), path
        assert open(path, "rb").read() == R.file_bytes(R.encode_frames(frames), G.duration_ms(9 if "result_full" in path else 3), 128, 64)
    assert handed[written.index(log["fullrate_paths"][0])].shape[0] == 7
