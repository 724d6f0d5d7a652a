"""The JPEG decoder on the CPU: the numpy restatement of the three stages (tests/_jpegdec_numpy.py) equals
Pillow byte for byte over the grid of tests/_jpegdec_cases.py — there is no tolerance —, the parser refuses what is outside the
subset and names why, the .avi route hands back decode_avi_u8's frames, the decode core of the kernel (csrc/jpegdec_core.h) runs the
grid and 2000 seeded corruptions clean under the host's sanitizers, and header, exports and binding agree."""
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image

import _jpegdec_cases as K
import _jpegdec_numpy as R
from ccedit_amd import jpegdec as J
from ccedit_amd import mjpeg as M

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ---- the restatement equals Pillow
def test_grid_is_the_issue_grid():
    names = [n for n, _ in K.grid()]
    assert len(names) == len(set(names)) == 7 * 4 * 4 * 2 * 2 * 4
    infos = [K.reference()[n][0] for n in names]
    assert {(i.ncomp, i.hs, i.vs) for i in infos} == {(3, 1, 1), (3, 2, 1), (3, 2, 2), (1, 1, 1)}
    assert any(len(i.intervals) == 10 for i in infos)                       # 160 x 16 at 4:2:0: RST0 ... RST7, RST0: the number wraps
    assert any(i.restart_interval == 0 for i in infos) and any(i.restart_interval > 0 for i in infos)
    std = tuple((bytes(bits), bytes(vals)) for _, _, bits, vals in (M.HUFFMAN[0], M.HUFFMAN[2], M.HUFFMAN[1], M.HUFFMAN[3]))
    colour = [i.huffman for i in infos if i.ncomp == 3]
    assert std in colour and any(h != std for h in colour)                  # default (Annex K) and optimised Huffman tables


def test_restatement_equals_pillow_over_the_grid():
    ref = K.reference()
    differ = [n for n, j in K.grid() if not np.array_equal(ref[n][3], K.pillow_decode(j))]
    assert not differ, f"{len(differ)} of {len(K.grid())} streams differ from Pillow, first {differ[:5]}"
    assert all(not ref[n][2].any() for n, _ in K.grid())


def test_restatement_equals_pillow_on_the_own_encoder():
    ref = K.reference()
    assert len(K.own_encoder()) == 8
    for n, j in K.own_encoder():
        assert np.array_equal(ref[n][3], K.pillow_decode(j)), n
        assert ref[n][0].restart_interval == 2 and len(ref[n][0].intervals) == 3           # one restart interval per MCU row


@pytest.mark.parametrize("w", [2, 3, 4, 5, 6])
@pytest.mark.parametrize("ss", ["4:2:2", "4:2:0"])
def test_narrow_planes(ss, w):
    """Chroma planes of one or two real columns are replicated, wider ones filtered (libjpeg chooses by the plane's width)."""
    j = K.pillow_jpeg(K.content("noise", 7, w, w), ss, 90, False, False)
    assert np.array_equal(R.decode(j), K.pillow_decode(j))


# ---- the parser
def _jpeg(**kw):
    b = io.BytesIO()
    Image.fromarray(K.content("noise", 24, 40, 5)).save(b, format="JPEG", quality=80, **kw)
    return b.getvalue()


def _segments(j):
    """-> list of (marker, offset, end) of the segments in front of the entropy-coded data."""
    out, at = [], 2
    while True:
        m, n = j[at + 1], struct.unpack_from(">H", j, at + 2)[0]
        out.append((m, at, at + 2 + n))
        at += 2 + n
        if m == 0xDA:
            return out


def test_parser_reads_the_layout():
    j = K.pillow_jpeg(K.content("ramp", 33, 50, 1), "4:2:0", 75, False, True)
    info = J.parse(j)
    assert (info.height, info.width, info.ncomp, info.hs, info.vs) == (33, 50, 3, 2, 2)
    assert (info.mcus_x, info.mcus_y, info.restart_interval, len(info.intervals)) == (4, 3, 4, 3)
    for k, (lo, hi) in enumerate(info.intervals.tolist()):
        assert j[hi:hi + 2] == (bytes([0xFF, 0xD0 + k]) if k < 2 else b"\xff\xd9")
    assert info.quant.shape == (3, 64)
    zz = next(j[a + 5:a + 69] for m, a, e in _segments(j) if m == 0xDB)
    assert info.quant[0, 8] == zz[2] and info.quant[0, 1] == zz[1]                   # natural order: zigzag place 2 is row 1, column 0


def test_parser_refusals():
    def refused(data, word):
        with pytest.raises(J.JpegUnsupported, match=word):
            J.parse(data)

    good = _jpeg()
    J.parse(good)
    refused(_jpeg(progressive=True), "progressive")
    b = io.BytesIO()
    Image.fromarray(K.content("noise", 16, 16, 1)).convert("CMYK").save(b, format="JPEG")
    refused(b.getvalue(), "CMYK")
    segs = _segments(good)
    for cut in (1, 3, segs[1][1] + 3, segs[-1][1] + 5, segs[-1][2] + 7, len(good) - 2, len(good) - 1):
        refused(good[:cut], "truncated|not a JPEG")
    dht = [(a, e) for m, a, e in segs if m == 0xC4]
    refused(good[:dht[0][0]] + good[dht[-1][1]:], "missing Huffman table")
    dqt = [(a, e) for m, a, e in segs if m == 0xDB]
    refused(good[:dqt[0][0]] + good[dqt[-1][1]:], "missing quantisation table")
    sof = next(a for m, a, e in segs if m == 0xC0)
    refused(good[:sof + 4] + b"\x0c" + good[sof + 5:], "12 bit")
    refused(good[:sof + 1] + b"\xc9" + good[sof + 2:], "arithmetic")
    refused(good[:sof + 11] + b"\x41" + good[sof + 12:], "sampling")                  # luma 4x1
    q16 = good[:dqt[0][0]] + b"\xff\xdb" + struct.pack(">HB", 2 + 129, 0x10) + bytes(128) + good[dqt[0][1]:]
    refused(q16, "16-bit quantisation")
    adobe = b"\xff\xee" + struct.pack(">H", 14) + b"Adobe\x00\x64\x00\x00\x00\x00\x00"
    app0 = segs[0]
    assert app0[0] == 0xE0
    refused(good[:2] + adobe + good[app0[2]:], "Adobe colour transform 0")
    sos = segs[-1]
    refused(good[:sos[1] + 4] + b"\x01" + good[sos[1] + 5:], "scan header|multiple scans")
    two = good[:-2] + good[sos[1]:]
    refused(two, "multiple scans")
    refused(good[:-2] + b"\xff\xd0\xff\xd9", "restart intervals|restart marker")
    assert issubclass(J.JpegUnsupported, ValueError)


def test_avi_route_hands_back_the_same_frames(tmp_path):
    frames = np.stack([K.content("noise", 48, 32, 3), K.content("ramp", 48, 32, 4)])
    import _mjpeg_numpy as E
    path = M.write_avi(str(tmp_path / "a.avi"), E.encode_frames(frames, 85), 8, 48, 32)
    jpegs = M.read_avi(path)[0]
    assert np.array_equal(np.stack([R.decode(j) for j in jpegs]), M.decode_avi_u8(path))


# ---- the decode core of the kernel, as a host program under the sanitizers
def _case(f, info, data, intervals, status, coef=None):
    f.write(struct.pack("<iiqqqqi", info.ncomp, info.hs * info.vs, info.mcus_x * info.mcus_y, info.mcus_per_interval, len(intervals),
                        len(data), int(coef is not None)))
    f.write(J.table_array(info).astype("<i4").tobytes())
    f.write(data)
    f.write(np.ascontiguousarray(intervals, "<i8").tobytes())
    f.write(np.ascontiguousarray(status, "<i4").tobytes())
    if coef is not None:
        f.write(np.ascontiguousarray(coef, "<i2").tobytes())


def test_decode_core_hardening(tmp_path):
    """The grid's streams decode to the restatement's coefficients, and 2000 seeded corruptions (byte flips, truncations, markers
    inserted inside the entropy-coded data) end every interval with the restatement's status: no read or write outside what the
    interval was given (AddressSanitizer), nothing undefined (UBSan), exit 0."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "jpegdec_harden")
    src = os.path.join(ROOT, "tests", "jpegdec_harden.cpp")
    clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout           # (c++ may be either)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libsan" if clang else "-static-libasan"]                                                  # (static: the runtime is part of the program)
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", *san, src, "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ref = K.reference()
    statuses = K.corruption_statuses()
    assert len(K.corruptions()) == 2000 and {int(s) for st in statuses for s in st} >= {0, 1, 2, 3}
    assert {c[0].rsplit("-", 1)[1].rstrip("0123456789") for c in K.corruptions()} == {"flip", "cut", "marker"}
    cases = str(tmp_path / "cases.bin")
    with open(cases, "wb") as f:
        n = len(K.grid()) + len(K.own_encoder()) + len(K.corruptions())
        f.write(b"JDH1" + struct.pack("<i", n))
        for name, j in K.grid() + K.own_encoder():
            info, coef, status, _ = ref[name]
            _case(f, info, j, info.intervals, status, coef)
        for (name, info, data, iv, _), status in zip(K.corruptions(), statuses):
            _case(f, info, data, iv, status)
    run = subprocess.run([exe, cases], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr.strip(), (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    assert f"{n} cases" in run.stdout and " 0 mismatches" in run.stdout, run.stdout


# ---- the C ABI: header, exports and binding agree (the conventions of tests/test_cabi.py)
def test_cabi_jpegdec():
    import ctypes
    import re
    from ccedit_amd import hip
    from ccedit_amd.csrc.build import build
    lib = ctypes.CDLL(build(force=False, verbose=False))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ccedit_hip.h")).read(), flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(ccedit_[a-z0-9_]+)\s*\(", src)) if n.startswith("ccedit_jpegdec_"))
    assert declared == ["ccedit_jpegdec_entropy", "ccedit_jpegdec_idct", "ccedit_jpegdec_plane_bytes", "ccedit_jpegdec_rgb"]
    for n in declared:
        assert hasattr(lib, n) and n in hip.EXPORTS
        args = re.search(re.escape(n) + r"\s*\(([^)]*)\)", src).group(1)
        assert len(hip._SIGS[n][1]) == len(args.split(",")), n
    assert "#define CCEDIT_ABI_VERSION 12" in src
    l = hip.lib()                                              # argument validation runs before any HIP call
    assert l.ccedit_jpegdec_plane_bytes(33, 50, 3, 2, 2) == 64 * 48 + 2 * 32 * 24
    assert l.ccedit_jpegdec_plane_bytes(33, 50, 1, 7, 7) == 56 * 40
    assert l.ccedit_jpegdec_plane_bytes(33, 50, 3, 1, 2) == -1 and b"sampling" in l.ccedit_last_error()
    assert l.ccedit_jpegdec_plane_bytes(0, 50, 3, 1, 1) == -1 and l.ccedit_jpegdec_plane_bytes(8, 65521, 1, 1, 1) == -1
    assert l.ccedit_jpegdec_entropy(None, 1, None, None, None, None, 1, 8, 8, 1, 1, 1, 0, None) == -1 and b"null" in l.ccedit_last_error()
    assert l.ccedit_jpegdec_entropy(16, 1, 16, 16, 16, 16, 1, 8, 8, 2, 1, 1, 0, None) == -1 and b"ncomp" in l.ccedit_last_error()
    assert l.ccedit_jpegdec_entropy(16, 0, 16, 16, 16, 16, 1, 8, 8, 1, 1, 1, 0, None) == -1 and b"data_bytes" in l.ccedit_last_error()
    assert l.ccedit_jpegdec_entropy(16, 1, 16, 16, 8, 16, 1, 8, 8, 1, 1, 1, 0, None) == -1 and b"aligned" in l.ccedit_last_error()
    assert l.ccedit_jpegdec_entropy(16, 1, 16, 16, 16, 16, 1, 8, 8, 1, 1, 1, -1, None) == -1 and b"restart_interval" in l.ccedit_last_error()
    assert l.ccedit_jpegdec_idct(16, 16, 12, 1, 8, 8, 1, 1, 1, None) == -1 and b"aligned" in l.ccedit_last_error()
    assert l.ccedit_jpegdec_idct(16, 16, 16, 0, 8, 8, 1, 1, 1, None) == -1 and b"N=0" in l.ccedit_last_error()
    assert l.ccedit_jpegdec_rgb(None, 16, 1, 8, 8, 1, 1, 1, None) == -1 and b"null" in l.ccedit_last_error()
    assert l.ccedit_jpegdec_rgb(16, 16, 1, 8, 70000, 1, 1, 1, None) == -1
    for call in (lambda: l.ccedit_jpegdec_rgb(16, 16, 40000, 256, 256, 1, 1, 1, None), lambda: l.ccedit_jpegdec_idct(16, 16, 16, 40000, 256, 256, 1, 1, 1, None)):
        assert call() == -1 and b"2^31 pixels" in l.ccedit_last_error()          # (within the plane and block bounds: one thread per pixel)
    assert J.TAB_SIZE == 3416 and (J.HUFF_STRIDE, J.TAB_HUFF) == (804, 200)
