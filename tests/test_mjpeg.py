"""Motion-JPEG output, the part that needs no GPU (ccedit_amd/mjpeg.py, --save_type mjpeg, tests/_mjpeg_numpy.py).

The numpy restatement is what the kernels must equal byte for byte (tests/test_mjpeg_gpu.py); here is what those bytes are worth:
every frame it produces decodes in Pillow with the right size, sampling and tables; its fidelity is Pillow's own encoder's with the
same tables to 0.1 dB; the container is walked chunk by chunk by a RIFF walker of this file; .avi files come back through the
loaders; the flags parse; the exports are declared, bound and refuse bad arguments before any HIP call.

On the stuffed-byte / ZRL requirement: uniform random bytes at q = 100 quantise with Q = 1 everywhere, so (nearly) every coefficient
is non-zero: the frame holds stuffed FF 00 bytes (asserted) but no run of 16 zeros, for any seed (seeds 0 ... 199 at 16 x 48 were
searched: none).  The ZRL symbol is asserted where the same random bytes do produce it, at q = 1 and q = 50, from the same trace."""
import io
import os
import re
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mjpeg_numpy as ref  # noqa: E402
from _mjpeg_images import IMAGES, QUALITIES, image, pil_decode, psnr  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SIZES = [(16, 16), (16, 48), (48, 32), (160, 16)]


# ---- tables and header -----------------------------------------------------------------------------
def test_quant_tables_follow_the_quality_rule():
    from ccedit_amd import mjpeg as M
    assert M.quant_tables(50) == (M.QUANT_LUMA.tolist(), M.QUANT_CHROMA.tolist())
    assert M.quant_tables(100) == ([1] * 64, [1] * 64)
    assert M.quant_tables(1)[0][0] == 255 and max(M.quant_tables(1)[1]) == 255
    assert M.quant_tables(90)[0][:4] == [3, 2, 2, 3] and M.quant_tables() == M.quant_tables(90)
    assert M.quant_tables(25)[0][0] == (16 * 200 + 50) // 100
    for bad in (0, 101, -3, 50.5):
        with pytest.raises(ValueError):
            M.quant_tables(bad)
    assert sorted(M.ZIGZAG.tolist()) == list(range(64))
    for tab in M.DC_CODES + M.AC_CODES:
        lens = tab & 255
        assert lens.max() <= 16 and np.sum(2.0 ** -lens[lens > 0].astype(np.float64)) < 1.0           # a prefix code with the all-ones word free
    assert (M.DC_CODES[0][:12] & 255).max() == 9 and (M.DC_CODES[1][:12] & 255).max() == 11
    assert np.count_nonzero(M.AC_CODES[0]) == 162 and np.count_nonzero(M.AC_CODES[1]) == 162
    assert M.table_array().shape == (M.TAB_SIZE,) and M.table_array().dtype == np.int32


def test_tables_are_the_ones_pillow_writes():
    """libjpeg carries the Annex K tables: its DHT segments and its quality-50 DQT are ours."""
    from PIL import Image
    from ccedit_amd import mjpeg as M

    def segments(b, marker):
        out, i = [], 2
        while i < len(b) and b[i + 1] != 0xDA:
            n = int.from_bytes(b[i + 2:i + 4], "big")
            if b[i + 1] == marker:
                out.append(b[i + 4:i + 2 + n])
            i += 2 + n
        return b"".join(out)

    def split_dht(d):
        t, i = {}, 0
        while i < len(d):
            n = sum(d[i + 1:i + 17])
            t[d[i]] = d[i + 1:i + 17 + n]
            i += 17 + n
        return t

    buf = io.BytesIO()
    Image.fromarray(image("gradient", 16, 16)).save(buf, "JPEG", quality=50, subsampling=2)
    assert split_dht(segments(buf.getvalue(), 0xC4)) == split_dht(segments(M.frame_header(16, 16, 50), 0xC4))
    q = pil_decode(buf.getvalue()).quantization
    assert (list(q[0]), list(q[1])) == M.quant_tables(50)


def test_header_layout():
    from ccedit_amd import mjpeg as M
    h = M.frame_header(48, 160, 75)
    assert h[:2] == b"\xff\xd8" and h[2:4] == b"\xff\xe0" and h[6:11] == b"JFIF\x00"
    order, i = [], 2
    while i < len(h):
        order.append(h[i + 1])
        n = int.from_bytes(h[i + 2:i + 4], "big")
        if h[i + 1] == 0xC0:
            assert struct.unpack(">BHHB", h[i + 4:i + 10]) == (8, 48, 160, 3) and h[i + 10:i + 19] == bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
        if h[i + 1] == 0xDD:
            assert struct.unpack(">H", h[i + 4:i + 6])[0] == 160 // 16
        i += 2 + n
    assert order == [0xE0, 0xDB, 0xC0, 0xC4, 0xDD, 0xDA] and i == len(h)
    for hw in ((40, 48), (48, 40), (0, 16), (16, 8)):
        with pytest.raises(ValueError, match=f"{hw[0]}x{hw[1]}"):
            M.frame_header(*hw)


# ---- the restatement decodes -----------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", IMAGES)
def test_restatement_decodes_in_pillow(name, size):
    from ccedit_amd import mjpeg as M
    h, w = size
    img = image(name, h, w)
    for q in QUALITIES:
        (jpeg,) = ref.encode_frames(img[None], q)
        assert jpeg[:2] == b"\xff\xd8" and jpeg[-2:] == b"\xff\xd9"
        im = pil_decode(jpeg)
        assert im.size == (w, h) and im.mode == "RGB"
        assert [tuple(l[1:3]) for l in im.layer] == [(2, 2), (1, 1), (1, 1)]
        assert (list(im.quantization[0]), list(im.quantization[1])) == M.quant_tables(q)
        rst = [jpeg[i + 1] for i in range(len(M.frame_header(h, w, q)), len(jpeg) - 2) if jpeg[i] == 0xFF and 0xD0 <= jpeg[i + 1] <= 0xD7]
        assert rst == [0xD0 + (r & 7) for r in range(h // 16 - 1)], "one RSTn between consecutive MCU rows, n cycling 0 ... 7"
        out = np.array(im)
        if name in ("black", "white"):
            assert np.abs(out.astype(int) - img.astype(int)).max() <= 1
        if name == "gradient" and q >= 90 and min(h, w) >= 32:
            assert psnr(out, img) > 35.0


def test_random_bytes_exercise_stuffing_and_zrl():
    stuffed, zrl = {}, {}
    for q in QUALITIES:
        tr = {}
        (jpeg,) = ref.encode_frames(image("random", 16, 48)[None], q, tr)
        stuffed[q], zrl[q] = tr.get("stuffed", 0), tr.get("zrl", 0)
        body = jpeg[jpeg.index(b"\xff\xda"):]
        assert body.count(b"\xff\x00") == stuffed[q]
        pil_decode(jpeg)
    print("stuffed", stuffed, "zrl", zrl)
    assert stuffed[100] >= 1, "the random-byte frame at q = 100 holds no stuffed FF 00"
    assert zrl[1] >= 1 and zrl[50] >= 1, "the random-byte frame holds no ZRL symbol at q = 1 / q = 50"
    tr = {}
    ref.encode_frames(image("halfflat", 16, 48)[None], 100, tr)
    assert tr.get("eob", 0) >= 1 and tr.get("stuffed", 0) >= 1


def test_restatement_does_not_depend_on_batching():
    frames = np.stack([image("smooth", 48, 32, s) for s in range(3)])
    together = ref.encode_frames(frames, 75)
    assert together == [ref.encode_frames(frames[i:i + 1], 75)[0] for i in range(3)] and len(set(together)) == 3


# ---- fidelity --------------------------------------------------------------------------------------
FIDELITY = {}


@pytest.mark.parametrize("q", [50, 90])
@pytest.mark.parametrize("name", ["gradient", "smooth"])
def test_fidelity_is_pillows_own(name, q):
    """Pillow's encoder with the same tables and sampling is the yardstick: ours may not be more than 0.1 dB below it."""
    from PIL import Image
    from ccedit_amd import mjpeg as M
    img = image(name, 64, 96)
    ours = psnr(np.array(pil_decode(ref.encode_frames(img[None], q)[0])), img)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", qtables=[list(t) for t in M.quant_tables(q)], subsampling=2)
    theirs_im = pil_decode(buf.getvalue())
    assert (list(theirs_im.quantization[0]), list(theirs_im.quantization[1])) == M.quant_tables(q)
    theirs = psnr(np.array(theirs_im), img)
    print(f"{name} q={q}: ours {ours:.3f} dB, Pillow {theirs:.3f} dB")
    assert ours >= theirs - 0.1, (ours, theirs)


# ---- container -------------------------------------------------------------------------------------
def riff_walk(data, at, end, depth=0):
    """-> [(fourcc, list kind or None, payload start, size, children)], checking that every chunk lies inside its parent, padded to even."""
    out = []
    while at < end:
        assert at + 8 <= end, "a chunk header runs past its parent"
        fourcc, size = data[at:at + 4], struct.unpack_from("<I", data, at + 4)[0]
        assert at + 8 + size <= end, (fourcc, at, size, end)
        if fourcc in (b"RIFF", b"LIST"):
            out.append((fourcc, data[at + 8:at + 12], at + 8, size, riff_walk(data, at + 12, at + 8 + size, depth + 1)))
        else:
            out.append((fourcc, None, at + 8, size, []))
        at += 8 + size + (size & 1)
        assert at % 2 == 0
    assert at == end, "padding or size does not add up"
    return out


def _jpegs(n, h, w, q=75):
    return ref.encode_frames(np.stack([image("smooth", h, w, s) for s in range(n)]), q)


def test_container_structure(tmp_path):
    from ccedit_amd import mjpeg as M
    h, w, n, fps = 32, 48, 5, 12
    jpegs = _jpegs(n, h, w)
    path = M.write_avi(str(tmp_path / "clip.avi"), jpegs, fps, h, w)
    data = open(path, "rb").read()
    (riff,) = riff_walk(data, 0, len(data))
    assert riff[0] == b"RIFF" and riff[1] == b"AVI " and riff[3] == len(data) - 8
    hdrl, movi, idx1 = riff[4]
    assert (hdrl[0], hdrl[1]) == (b"LIST", b"hdrl") and (movi[0], movi[1]) == (b"LIST", b"movi") and idx1[0] == b"idx1"
    avih, strl = hdrl[4]
    assert avih[0] == b"avih" and avih[3] == 56 and (strl[0], strl[1]) == (b"LIST", b"strl")
    a = struct.unpack_from("<14I", data, avih[2])
    assert a[0] == 1000000 // fps and a[4] == n and a[6] == 1 and (a[8], a[9]) == (w, h) and a[3] & 0x10
    strh, strf = strl[4]
    assert strh[0] == b"strh" and strh[3] == 56 and strf[0] == b"strf" and strf[3] == 40
    assert data[strh[2]:strh[2] + 8] == b"vidsMJPG"
    scale, rate, _, length = struct.unpack_from("<IIII", data, strh[2] + 20)
    assert rate / scale == fps and scale == 1 and length == n
    assert struct.unpack_from("<hhhh", data, strh[2] + 48) == (0, 0, w, h)
    bi = struct.unpack_from("<IiiHH4sI", data, strf[2])
    assert bi == (40, w, h, 1, 24, b"MJPG", w * h * 3)
    chunks = movi[4]
    assert len(chunks) == n and all(c[0] == b"00dc" for c in chunks)
    assert [data[c[2]:c[2] + c[3]] for c in chunks] == jpegs
    assert idx1[3] == 16 * n
    for i in range(n):
        cid, flags, off, size = struct.unpack_from("<4sIII", data, idx1[2] + 16 * i)
        at = movi[2] + off                                       # offsets count from the `movi` fourcc
        assert cid == b"00dc" and flags & 0x10 and data[at:at + 4] == b"00dc" and struct.unpack_from("<I", data, at + 4)[0] == size == len(jpegs[i])
        assert data[at + 8:at + 10] == b"\xff\xd8" and data[at + 8 + size - 2:at + 8 + size] == b"\xff\xd9"
    assert any(len(j) & 1 for j in jpegs) and any(not len(j) & 1 for j in jpegs), "both paddings exercised"


def test_container_round_trip_and_refusals(tmp_path):
    from ccedit_amd import mjpeg as M
    jpegs = _jpegs(3, 16, 32)
    path = M.write_avi(str(tmp_path / "a.avi"), jpegs, 7, 16, 32)
    assert M.read_avi(path) == (jpegs, 7, 16, 32)
    data = bytearray(open(path, "rb").read())
    other = bytes(data).replace(b"MJPG", b"H264")
    open(str(tmp_path / "h264.avi"), "wb").write(other)
    with pytest.raises(ValueError, match="H264"):
        M.read_avi(str(tmp_path / "h264.avi"))
    open(str(tmp_path / "cut.avi"), "wb").write(bytes(data[:len(data) // 2]))
    with pytest.raises(ValueError, match="truncated"):
        M.read_avi(str(tmp_path / "cut.avi"))
    with pytest.raises(ValueError, match="no such"):
        M.read_avi(str(tmp_path / "missing.avi"))
    open(str(tmp_path / "text.avi"), "wb").write(b"not a video")
    with pytest.raises(ValueError, match="RIFF"):
        M.read_avi(str(tmp_path / "text.avi"))
    with pytest.raises(ValueError):
        M.write_avi(str(tmp_path / "b.avi"), [], 7, 16, 32)
    with pytest.raises(ValueError, match="fps"):
        M.write_avi(str(tmp_path / "b.avi"), jpegs, 0, 16, 32)


def test_two_gib_is_refused_before_anything_is_written(tmp_path):
    from ccedit_amd import mjpeg as M

    class Big(bytes):
        def __len__(self):
            return 2 ** 30

    with pytest.raises(ValueError, match="2 GiB"):
        M.write_avi(str(tmp_path / "big.avi"), [Big(b"x")] * 2, 10, 16, 16)
    assert not os.path.exists(str(tmp_path / "big.avi"))


# ---- loaders ---------------------------------------------------------------------------------------
def test_avi_is_a_video_source(tmp_path):
    from ccedit_amd import mjpeg as M
    from scripts.sampling.util import count_video_frames, keyframe_indices, load_video_keyframes, load_video_mask
    n, h, w = 10, 32, 48
    frames = np.stack([image("smooth", h, w, s) for s in range(n)])
    jpegs = ref.encode_frames(frames, 90)
    path = M.write_avi(str(tmp_path / "clip.avi"), jpegs, 12, h, w)
    assert count_video_frames(path) == n
    idx = keyframe_indices(n, 12, 4, 3)
    assert idx.tolist() == [0, 3, 6]
    decoded = np.stack([np.array(pil_decode(jpegs[i])) for i in idx])
    kf = load_video_keyframes(path, 12, 4, 3)
    assert tuple(kf.shape) == (3, 3, h, w)
    want = np.clip(decoded.transpose(0, 3, 1, 2).astype(np.float32) / 255.0 * 2.0 - 1.0, -1.0, 1.0)
    assert np.array_equal(kf.numpy(), want)
    assert psnr(decoded, frames[idx]) > 25.0
    assert tuple(load_video_keyframes(path, 12, 4, 3, (16, 24)).shape) == (3, 3, 16, 24)
    white = np.zeros((n, h, w, 3), np.uint8)
    for i in range(n):
        white[i, :, 4 * i:] = 255
    mpath = M.write_avi(str(tmp_path / "mask.avi"), ref.encode_frames(white, 90), 12, h, w)
    m = load_video_mask(mpath, 12, 4, 3, None, n)
    assert tuple(m.shape) == (3, h, w) and [int((m[k, 0] == 0).sum()) for k in range(3)] == [0, 12, 24]
    assert tuple(load_video_mask(mpath, 12, 4, 3, None, n, all_frames=True).shape) == (n, h, w)
    with pytest.raises(ValueError):
        load_video_keyframes(str(tmp_path / "nothing.avi"), 12, 4, 3)
    with pytest.raises(ValueError):
        count_video_frames(str(tmp_path / "nothing.avi"))


# ---- arguments -------------------------------------------------------------------------------------
def test_flags_parse_in_both_scripts(capsys):
    from scripts.sampling import sampling_tv2v as S
    from scripts.sampling import sampling_tv2v_ref as R
    for mod in (S, R):
        a = mod.parse_args([])
        assert a.save_type == "npy" and a.video_quality == 90
        a = mod.parse_args(["--save_type", "mjpeg", "--video_quality", "75"])
        assert a.save_type == "mjpeg" and a.video_quality == 75
        for bad in ("0", "101"):
            with pytest.raises(SystemExit):
                mod.parse_args(["--save_type", "mjpeg", "--video_quality", bad])
            assert "--video_quality" in capsys.readouterr().err
        with pytest.raises(SystemExit):
            mod.parse_args(["--save_type", "mjpeg", "--H", "72"])
        assert "multiples of 16" in capsys.readouterr().err
    helps = {act.dest: act.help for act in S.make_parser()._actions}
    assert "mjpeg" in helps["save_type"] and "(not in the reference script)" in helps["video_quality"]


def test_propagate_accepts_mjpeg(tmp_path, capsys):
    from PIL import Image
    from scripts.sampling import sampling_tv2v as S
    vdir = tmp_path / "fox"
    vdir.mkdir()
    for i in range(5):
        Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(str(vdir / f"{i:03d}.png"))
    args = S.parse_args(["--propagate", "--save_type", "mjpeg", "--prompt", "a fox", "--video_path", str(vdir), "--num_keyframes", "2",
                         "--original_fps", "4", "--target_fps", "1"])
    assert args.propagate and args.save_type == "mjpeg"
    S.check_propagate(args, [str(vdir)])
    with pytest.raises(SystemExit):
        S.parse_args(["--propagate", "--save_type", "npy", "--prompt", "a fox", "--video_path", str(vdir)])
    err = capsys.readouterr().err
    assert "--save_type gif" in err and "mjpeg" in err
    # an .avi source is counted and planned like a .gif one
    from ccedit_amd import mjpeg as M
    path = M.write_avi(str(tmp_path / "clip.avi"), _jpegs(5, 16, 16), 4, 16, 16)
    S.check_propagate(S.parse_args(["--propagate", "--save_type", "mjpeg", "--prompt", "a fox", "--video_path", path, "--num_keyframes", "2",
                                    "--original_fps", "4", "--target_fps", "1"]), [path])
    with pytest.raises(ValueError, match="lower --num_keyframes"):
        S.check_propagate(S.parse_args(["--propagate", "--save_type", "mjpeg", "--prompt", "a fox", "--video_path", path, "--num_keyframes", "9"]),
                          [path])


def test_mp4_and_gpu_io_refusals_are_unchanged():
    import torch
    from scripts.sampling.util import perform_save_locally_video
    x = torch.zeros(1, 3, 2, 16, 16)
    with pytest.raises(NotImplementedError, match="mp4 encoding needs"):
        perform_save_locally_video("unused", x, 3, "mp4")
    for st in ("gif", "mjpeg", "npy"):
        with pytest.raises(ValueError, match=r"gpu_io saves uint8 frames \(savetype='gif'\) of a device tensor"):
            perform_save_locally_video("unused", x, 3, st, gpu_io=True)


# ---- exports ---------------------------------------------------------------------------------------
NEW = ("ccedit_mjpeg_segment_bytes", "ccedit_mjpeg_transform", "ccedit_mjpeg_entropy", "ccedit_mjpeg_pack_scan", "ccedit_mjpeg_pack")


def test_new_exports_are_declared_and_bound():
    from ccedit_amd import hip, ops
    src = open(os.path.join(ROOT, "include", "ccedit_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", code), f"{name} is not declared in include/ccedit_hip.h"
        assert name in hip.EXPORTS
        assert hasattr(ops, name[len("ccedit_"):])
    assert hip.ABI_VERSION == 12 and "#define CCEDIT_ABI_VERSION 12" in src
    assert hip.lib().ccedit_abi_version() == 12
    build = open(os.path.join(ROOT, "ccedit_amd", "csrc", "build.py")).read()
    assert '"mjpeg.hip": ["-ffp-contract=off", "-fno-slp-vectorize"]' in build


def test_segment_bytes_hold_the_worst_case():
    from ccedit_amd import hip
    from ccedit_amd import mjpeg as M
    lib = hip.lib()
    for w in (16, 48, 768, 65520):
        blocks = w // 16 * 6
        cap = lib.ccedit_mjpeg_segment_bytes(w)
        assert cap % 16 == 0 and cap >= 2 * ((blocks * M.MAX_BLOCK_BITS + 7) // 8 + 1)
    assert lib.ccedit_mjpeg_segment_bytes(40) == -1 and b"multiple of 16" in lib.ccedit_last_error()
    assert M.MAX_BLOCK_BITS >= 63 * 26 + 20


def test_entry_points_report_bad_arguments():
    """Argument validation runs before any HIP call (pointer stand-ins, as tests/test_propagate.py does)."""
    from ccedit_amd import hip
    lib = hip.lib()
    err = lambda: lib.ccedit_last_error()
    # transform(frames, tables, coef, N, H, W, quality, stream)
    assert lib.ccedit_mjpeg_transform(None, 16, 16, 1, 16, 16, 90, None) == -1 and b"null" in err() and b"frames" in err()
    assert lib.ccedit_mjpeg_transform(16, None, 16, 1, 16, 16, 90, None) == -1 and b"null" in err()
    assert lib.ccedit_mjpeg_transform(16, 16, None, 1, 16, 16, 90, None) == -1 and b"null" in err()
    assert lib.ccedit_mjpeg_transform(16, 16, 16, 0, 16, 16, 90, None) == -1 and b"N=0" in err()
    assert lib.ccedit_mjpeg_transform(16, 16, 16, 1, 24, 16, 90, None) == -1 and b"24x16" in err() and b"multiples of 16" in err()
    assert lib.ccedit_mjpeg_transform(16, 16, 16, 1, 16, 40, 90, None) == -1 and b"16x40" in err()
    assert lib.ccedit_mjpeg_transform(16, 16, 16, 1, 16, 16, 0, None) == -1 and b"quality=0" in err()
    assert lib.ccedit_mjpeg_transform(16, 16, 16, 1, 16, 16, 101, None) == -1 and b"quality=101" in err()
    assert lib.ccedit_mjpeg_transform(24, 16, 16, 1, 16, 16, 90, None) == -1 and b"aligned" in err() and b"frames" in err()
    assert lib.ccedit_mjpeg_transform(16, 16, 24, 1, 16, 16, 90, None) == -1 and b"aligned" in err()
    assert lib.ccedit_mjpeg_transform(16, 18, 16, 1, 16, 16, 90, None) == -1 and b"aligned" in err()
    # entropy(coef, tables, segments, seg_len, N, H, W, stream)
    assert lib.ccedit_mjpeg_entropy(16, 16, 16, None, 1, 16, 16, None) == -1 and b"null" in err()
    assert lib.ccedit_mjpeg_entropy(16, 16, 16, 16, -1, 16, 16, None) == -1 and b"N=-1" in err()
    assert lib.ccedit_mjpeg_entropy(16, 16, 16, 16, 1, 16, 8, None) == -1 and b"multiples of 16" in err()
    assert lib.ccedit_mjpeg_entropy(8, 16, 16, 16, 1, 16, 16, None) == -1 and b"coef" in err() and b"aligned" in err()
    assert lib.ccedit_mjpeg_entropy(16, 16, 16, 18, 1, 16, 16, None) == -1 and b"seg_len" in err()
    # pack_scan(seg_len, seg_off, frame_bytes, N, H, W, hdr_len, stream)
    assert lib.ccedit_mjpeg_pack_scan(16, None, 16, 1, 16, 16, 600, None) == -1 and b"null" in err()
    assert lib.ccedit_mjpeg_pack_scan(16, 16, 16, 0, 16, 16, 600, None) == -1 and b"N=0" in err()
    assert lib.ccedit_mjpeg_pack_scan(16, 16, 16, 1, 16, 17, 600, None) == -1 and b"multiples of 16" in err()
    assert lib.ccedit_mjpeg_pack_scan(16, 16, 16, 1, 16, 16, 0, None) == -1 and b"hdr_len" in err()
    assert lib.ccedit_mjpeg_pack_scan(16, 20, 16, 1, 16, 16, 600, None) == -1 and b"seg_off" in err()
    # pack(segments, seg_len, seg_off, header, out, N, H, W, hdr_len, out_bytes, stream)
    assert lib.ccedit_mjpeg_pack(16, 16, 16, None, 16, 1, 16, 16, 600, 1000, None) == -1 and b"null" in err()
    assert lib.ccedit_mjpeg_pack(16, 16, 16, 16, 16, 0, 16, 16, 600, 1000, None) == -1 and b"N=0" in err()
    assert lib.ccedit_mjpeg_pack(16, 16, 16, 16, 16, 1, 20, 16, 600, 1000, None) == -1 and b"multiples of 16" in err()
    assert lib.ccedit_mjpeg_pack(16, 16, 16, 16, 16, 1, 16, 16, 600, 100, None) == -1 and b"out_bytes" in err()
    assert lib.ccedit_mjpeg_pack(16, 18, 16, 16, 16, 1, 16, 16, 600, 1000, None) == -1 and b"seg_len" in err()
