"""PNG sources decoded on a real MI355X (ccedit_amd/pngdec.py, csrc/pngdec.hip).

Exact (no tolerance anywhere): the inflate stage against zlib.decompress, the unfilter stage against the reference of
tests/_pngdec_cases.py, whole files against Pillow, over the grid of tests/_pngdec_cases.py; independence of the scratch budget;
`select`; the entry level (frame directory, one image, animated .png) against the Pillow route.  LAST: the documented invalid streams,
each run through the sanitizer-built host core first, which must stop with their statuses and write nothing outside their buffers."""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pngdec_cases as K  # noqa: E402
import _png_numpy as M  # noqa: E402
from ccedit_amd import png as P  # noqa: E402

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _by_size():
    sizes = {}
    for name, (h, w, _, _) in K.all_streams().items():
        sizes.setdefault((h, w), []).append(name)
    return sizes


def _inflate(streams, h, w):
    from ccedit_amd import ops, pngdec
    data, table = pngdec.pack_streams(streams)
    filtered, status = ops.pngdec_inflate(torch.from_numpy(data).cuda(), torch.from_numpy(table).cuda(), h, w)
    return filtered.cpu().numpy(), status.cpu().numpy()


def _pillow_frames(data: bytes) -> np.ndarray:
    from PIL import Image, ImageSequence
    return np.stack([np.array(fr.convert("RGB")) for fr in ImageSequence.Iterator(Image.open(io.BytesIO(data)))])


# ---- 1. the stages ---------------------------------------------------------------------------------
def test_inflate_equals_zlib_over_the_grid():
    """Every stream of the grid and the crafted ones, in calls of 1, 3 and 17 streams of unequal compressed length (then the rest)."""
    _need_gpu()
    S = K.all_streams()
    seen, calls, unequal = 0, set(), set()
    for (h, w), names in _by_size().items():
        at = 0
        for n in (1, 3, 17, len(names)):
            part = names[at:at + n]
            at += len(part)
            if not part:
                continue
            got, status = _inflate([S[k][3] for k in part], h, w)
            assert not status.any(), (h, w, part, status)
            for i, k in enumerate(part):
                assert got[i].tobytes() == S[k][2], k
            seen += len(part)
            calls.add(len(part))
            if len({len(S[k][3]) for k in part}) > 1:
                unequal.add(len(part))
    assert seen == len(S) == 763 and calls >= {1, 3, 17} and unequal >= {3, 17}


def test_unfilter_equals_the_reference_on_random_bytes():
    _need_gpu()
    from ccedit_amd import ops
    rs = np.random.RandomState(5)
    for h in K.HEIGHTS:
        for w in K.WIDTHS:
            f = rs.randint(0, 256, size=(3, h, 1 + 3 * w)).astype(np.uint8)
            f[:, :, 0] = rs.randint(0, 5, size=(3, h))
            got, status = ops.pngdec_unfilter(torch.from_numpy(f.reshape(3, -1)).cuda(), h, w)
            assert not status.cpu().numpy().any()
            got = got.cpu().numpy()
            for i in range(3):
                assert np.array_equal(got[i], K.unfilter(f[i].tobytes(), h, w)), (h, w, i)


# ---- 2. whole files --------------------------------------------------------------------------------
def test_decode_equals_pillow_over_the_grid():
    """Per size all files in one decode call, and all streams as the frames of one animated file through decode_apng."""
    _need_gpu()
    from ccedit_amd import pngdec
    S = K.all_streams()
    for (h, w), names in _by_size().items():
        files = [K.png_file(h, w, [S[k][3]], idat_bytes=1 if i % 7 == 3 and len(S[k][3]) < 3000 else None) for i, k in enumerate(names)]
        want = np.stack([K.pillow_decode(f) for f in files])
        got = pngdec.decode(files, "cuda")
        assert got.dtype == torch.uint8 and tuple(got.shape) == (len(names), h, w, 3)
        assert np.array_equal(got.cpu().numpy(), want), (h, w)
        if len(names) > 1:
            anim = K.png_file(h, w, [S[k][3] for k in names])
            assert np.array_equal(pngdec.decode_apng(anim, "cuda").cpu().numpy(), _pillow_frames(anim)), (h, w)
            assert np.array_equal(_pillow_frames(anim), want)
    with pytest.raises(ValueError, match="different sizes"):
        pngdec.decode([K.png_file(1, 1, [S["1x1-f0-l6"][3]]), K.png_file(2, 1, [S["2x1-f0-l6"][3]])], "cuda")
    with pytest.raises(ValueError, match="no frames"):
        pngdec.decode([], "cuda")


def test_clip_and_full_size_frames_for_two_scratch_budgets(tmp_path, monkeypatch):
    """17 frames of 128 x 192 (Pillow's writer and the own encoder's file), one 512 x 768 frame from each: equal to Pillow, and the
    same whether all frames share one launch or every frame has its own."""
    _need_gpu()
    from ccedit_amd import pngdec
    frames = np.stack([K.image(128, 192, 20 + i) for i in range(17)])
    files = [K.pillow_png(f, optimize=bool(i & 1)) for i, f in enumerate(frames)]
    anim = open(P.write_apng(str(tmp_path / "own.png"), M.encode_frames(frames[:5]), 100, 192, 128), "rb").read()
    big = K.image(512, 768, 2).copy()                       # a ramp below a photo-like band: the restatement codes long matches quickly
    big[:160] = K.image(160, 768, 4)
    big_files = [K.pillow_png(big, False), K.png_file(512, 768, [M.zlib_stream(M.filter_frame(big).tobytes())])]
    outs = []
    for budget in (pngdec.SCRATCH_BYTES, 1):
        monkeypatch.setattr(pngdec, "SCRATCH_BYTES", budget)
        assert pngdec.frames_per_launch(128, 192) == (256 if budget > 1 else 1)
        outs.append((pngdec.decode(files, "cuda").cpu().numpy(), pngdec.decode_apng(anim, "cuda").cpu().numpy(),
                     pngdec.decode(big_files, "cuda").cpu().numpy()))
    for a, b, c in outs:
        assert np.array_equal(a, frames) and np.array_equal(b, frames[:5]) and np.array_equal(c, np.stack([big, big]))
    assert np.array_equal(_pillow_frames(anim), frames[:5]) and np.array_equal(K.pillow_decode(big_files[1]), big)


def test_select_decodes_only_the_chosen_frames(tmp_path, monkeypatch):
    _need_gpu()
    from ccedit_amd import ops, pngdec
    frames = np.stack([K.image(33, 50, 60 + i) for i in range(9)])
    anim = open(P.write_apng(str(tmp_path / "a.png"), M.encode_frames(frames), 100, 50, 33), "rb").read()
    everything = pngdec.decode_apng(anim, "cuda")
    launched = []
    real = ops.pngdec_inflate
    monkeypatch.setattr(ops, "pngdec_inflate", lambda d, t, h, w: (launched.append(t.shape[0]), real(d, t, h, w))[1])
    asked = []
    got = pngdec.decode_apng(anim, "cuda", select=lambda n: (asked.append(n), [7, 0, 4, 4])[1])
    assert asked == [9] and launched == [4]
    assert torch.equal(got, everything[[7, 0, 4, 4]]) and np.array_equal(everything.cpu().numpy(), frames)
    with pytest.raises(ValueError, match="frame indices"):
        pngdec.decode_apng(anim, "cuda", select=lambda n: [n])


# ---- 3. the entry level ----------------------------------------------------------------------------
def _refuse(monkeypatch):
    from ccedit_amd import pngdec

    def parse(data):
        raise pngdec.PngUnsupported("refused by the test")
    monkeypatch.setattr(pngdec, "parse", parse)


def _count_launches(monkeypatch):
    from ccedit_amd import ops
    calls = []
    real = ops.pngdec_unfilter
    monkeypatch.setattr(ops, "pngdec_unfilter", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def test_directory_and_image_loaders_equal_the_pillow_route(tmp_path, monkeypatch, capfd):
    """load_video_keyframes and load_video_frames_u8 on a directory of seven 128 x 192 .png files at (64, 96), load_img on one .png: the
    device decoder and _decode_rgb_u8 + upload give the same tensors, bit for bit; an unsupported file in the directory sends the
    whole clip through Pillow with one line on stderr, and the tensors are the same again."""
    _need_gpu()
    from PIL import Image
    from scripts.sampling import util as U
    vdir = tmp_path / "frames"
    vdir.mkdir()
    imgs = [K.image(128, 192, 80 + i) for i in range(7)]
    for i, im in enumerate(imgs):
        Image.fromarray(im).save(str(vdir / f"{i:03d}.png"), optimize=bool(i & 1))
    calls = _count_launches(monkeypatch)

    def load():
        return (U.load_video_keyframes(str(vdir), 6, 3, 3, (64, 96), device="cuda").cpu(), U.load_video_frames_u8(str(vdir), (64, 96), "cuda").cpu(),
                U.load_img(str(vdir / "002.png"), (64, 96), device="cuda").cpu(), U.load_img(str(vdir / "002.png"), None, device="cuda").cpu())
    device = load()
    assert len(calls) == 4 and capfd.readouterr().err == ""
    assert tuple(device[0].shape) == (3, 3, 64, 96) and tuple(device[1].shape) == (7, 64, 96, 3) and tuple(device[3].shape) == (1, 3, 128, 192)
    with monkeypatch.context() as m:
        _refuse(m)
        pillow = load()
    assert len(calls) == 4, "the forced Pillow route launched the decoder"
    assert capfd.readouterr().err.count("refused by the test") == 4
    for a, b in zip(device, pillow):
        assert torch.equal(a, b)
    # an unsupported file among the keyframes (files 0, 2, 4): an Adam7-interlaced copy of the same pixels
    (vdir / "004.png").write_bytes(_interlaced(imgs[4]))
    assert np.array_equal(K.pillow_decode(open(str(vdir / "004.png"), "rb").read()), imgs[4])
    for k, fn in enumerate((lambda: U.load_video_keyframes(str(vdir), 6, 3, 3, (64, 96), device="cuda"),
                            lambda: U.load_video_frames_u8(str(vdir), (64, 96), "cuda"))):
        odd = fn().cpu()
        err = capfd.readouterr().err
        assert len(calls) == 4 and err.count("\n") == 1 and err.startswith("[pngdec] ") and "004.png: Adam7" in err
        assert err.endswith("this clip is decoded by Pillow on the host\n")
        assert torch.equal(odd, device[k])


def _interlaced(img: np.ndarray) -> bytes:
    """An Adam7-interlaced 8-bit RGB PNG of the image, written by hand (Pillow's writer does not interlace): filter 0 throughout."""
    import struct
    import zlib
    h, w, _ = img.shape
    raw = bytearray()
    for y0, x0, dy, dx in ((0, 0, 8, 8), (0, 4, 8, 8), (4, 0, 8, 4), (0, 2, 4, 4), (2, 0, 4, 2), (0, 1, 2, 2), (1, 0, 2, 1)):
        sub = img[y0::dy, x0::dx]
        if sub.shape[0] and sub.shape[1]:
            for row in sub:
                raw += b"\0" + row.tobytes()
    return (P.SIGNATURE + P._chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 1)) + P._chunk(b"IDAT", zlib.compress(bytes(raw)))
            + P._chunk(b"IEND", b""))


def test_animated_png_equals_the_gif_route(tmp_path, monkeypatch, capfd):
    """An animated .png (8 frames of 128 x 192, the own encoder's file) through both loaders, at its own size and at (64, 96): the device
    decoder and Pillow's route, the .gif's, (the parser made to refuse) give the same tensors, frame for frame."""
    _need_gpu()
    from scripts.sampling import util as U
    frames = np.stack([K.image(128, 192, 30 + i) for i in range(8)])
    path = P.write_apng(str(tmp_path / "clip.png"), M.encode_frames(frames), 125, 192, 128)
    from ccedit_amd import video_io
    assert video_io.kind_of(path) is video_io.APNG and U.count_video_frames(path) == 8
    calls = _count_launches(monkeypatch)

    def load():
        return [U.load_video_keyframes(path, 6, 3, 3, size, device="cuda").cpu() for size in (None, (64, 96))] + \
               [U.load_video_frames_u8(path, size, "cuda").cpu() for size in ((128, 192), (64, 96))]
    device = load()
    assert len(calls) == 4 and capfd.readouterr().err == ""
    with monkeypatch.context() as m:
        _refuse(m)
        pillow = load()
    assert len(calls) == 4 and capfd.readouterr().err.count("decoded by Pillow on the host") == 4
    assert [tuple(t.shape) for t in device] == [(3, 3, 128, 192), (3, 3, 64, 96), (8, 128, 192, 3), (8, 64, 96, 3)]
    for a, b in zip(device, pillow):
        assert torch.equal(a, b)


# ---- 4. LAST: invalid streams ----------------------------------------------------------------------
GUARD = 4096


def _guarded(nbytes: int, dtype=torch.uint8):
    """-> (the whole buffer filled with 0xA5, the view of `nbytes` bytes in its middle)"""
    whole = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD:GUARD + nbytes]


def _guards_intact(whole) -> bool:
    a = whole.cpu().numpy()
    return bool((a[:GUARD] == 0xA5).all() and (a[-GUARD:] == 0xA5).all())


def test_zz_invalid_streams_stop_with_their_statuses():
    """A stream cut in the middle, a wrong Adler-32, a distance before the start, an output one byte too long and one byte too short:
    each was first run through the sanitizer-built host core (tests/pngdec_harden.cpp), which stopped with the documented status.  On
    the device, between two good streams of the same call, each stops with the same status and position, the good streams decode, and
    the guard bytes around the output and the status buffer are unchanged.  Then a filter byte 5 in the unfilter stage."""
    _need_gpu()
    from ccedit_amd import hip, pngdec
    lib = hip.lib()
    inv = K.invalid_streams()
    host = K.run_host_core([(h, w, z, None, None) for h, w, z, _, _ in inv.values()])            # FIRST: the host core, under the sanitizers
    S = K.all_streams()
    for (name, (h, w, z, code, where)), (hc, hp) in zip(inv.items(), host.tolist()):
        assert hc == code and (where is None or hp == where), (name, hc, hp)
        good = [S[k] for k in _by_size()[(h, w)][:2]]
        L = P.filtered_bytes(h, w)
        data, table = pngdec.pack_streams([good[0][3], z, good[1][3]])
        d, t = torch.from_numpy(data).cuda(), torch.from_numpy(table).cuda()
        out_whole, out = _guarded(3 * L)
        st_whole, st = _guarded(3 * 2 * 4)
        rc = lib.ccedit_pngdec_inflate(d.data_ptr(), d.numel(), t.data_ptr(), out.data_ptr(), st.data_ptr(), 3, h, w,
                                       torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.ccedit_last_error()
        torch.cuda.synchronize()
        status = st.cpu().numpy().view(np.int32).reshape(3, 2)
        assert status.tolist() == [[0, 0], [hc, hp], [0, 0]], (name, status)
        got = out.cpu().numpy().reshape(3, L)
        assert got[0].tobytes() == good[0][2] and got[2].tobytes() == good[1][2], name
        assert _guards_intact(out_whole) and _guards_intact(st_whole), name
        with pytest.raises(ValueError, match=rf"frame 1: .*\(code {code} at byte {hp}\)") as e:
            pngdec.decode_streams([good[0][3], z, good[1][3]], h, w, "cuda")
        assert not isinstance(e.value, pngdec.PngUnsupported)
        rgb, status = pngdec.decode_streams([good[0][3], z, good[1][3]], h, w, "cuda", check=False)
        assert status.tolist() == [[0, 0], [hc, hp], [0, 0]]
        assert np.array_equal(rgb[0].cpu().numpy(), K.unfilter(good[0][2], h, w)) and np.array_equal(rgb[2].cpu().numpy(), K.unfilter(good[1][2], h, w))
    h, w, f, at = K.filter_byte_five()
    assert K.run_host_core([(h, w, None, f, None)]).tolist() == [[12, at]]
    ok = K.filter_rows(K.image(h, w, 8), K.filter_types("cycle", h))
    fd = torch.from_numpy(np.frombuffer(ok + f + ok, np.uint8).copy()).cuda()
    out_whole, out = _guarded(3 * h * w * 3)
    st_whole, st = _guarded(3 * 2 * 4)
    assert lib.ccedit_pngdec_unfilter(fd.data_ptr(), out.data_ptr(), st.data_ptr(), 3, h, w, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert st.cpu().numpy().view(np.int32).reshape(3, 2).tolist() == [[0, 0], [12, at], [0, 0]]
    got = out.cpu().numpy().reshape(3, h, w, 3)
    assert np.array_equal(got[0], K.image(h, w, 8)) and np.array_equal(got[2], K.image(h, w, 8))
    assert np.array_equal(got[1, :64], K.unfilter(f[:64 * (1 + 3 * w)], 64, w))              # the band before the one that holds row 70
    assert _guards_intact(out_whole) and _guards_intact(st_whole)
    bad_file = K.png_file(h, w, [K.compress(f, "l6")])
    with pytest.raises(ValueError, match=rf"frame 0: a filter byte above 4 \(code 12 at byte {at}\)"):
        pngdec.decode([bad_file], "cuda")
    with pytest.raises(OSError):
        K.pillow_decode(bad_file)
