"""The PNG decoder on the CPU: the parser reads layout, frame count and payloads of every case of
tests/_pngdec_cases.py and refuses what is outside the subset by name; the core of the kernels (csrc/pngdec_core.h), built as a host
program under the sanitizers, reproduces zlib.decompress and the unfilter reference over the whole grid and ends 2000 seeded
corruptions with a status or a correct image; header, exports and binding agree; the routing declines what it must without a device."""
import io
import os
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

import _pngdec_cases as K
import _png_numpy as M
from ccedit_amd import png as P
from ccedit_amd import pngdec as D

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ---- the generator
def test_grid_is_the_issue_grid():
    g = K.grid()
    assert len(g) == 5 * 5 * 6 * 5
    assert {P.row_bytes(w) for w in K.WIDTHS} == {4, 7, 64, 256, 577} and K.HEIGHTS == (1, 2, 64, 65, 130)
    for name, (h, w, filtered, z) in K.all_streams().items():
        assert len(filtered) == P.filtered_bytes(h, w) and zlib.decompress(z) == filtered, name
    first_block = lambda z: (z[2] >> 1) & 3                                           # noqa: E731
    assert {first_block(g[f"64x85-cycle-{k}"][3]) for k in K.KINDS} == {0, 1, 2}
    assert first_block(g["64x85-cycle-stored"][3]) == 0 and first_block(g["64x85-cycle-fixed"][3]) == 1
    c = K.crafted()
    assert len(c["noise-mixed-blocks"][2]) > 65536 and first_block(c["noise-mixed-blocks"][3]) == 0
    assert c["far-distance-32768"][2][32768:] == c["far-distance-32768"][2][:4096]
    assert len(c["zeros-l9-overlapping-copies"][3]) < 100
    for name in g:
        h, _, filtered, _ = g[name]
        rb = len(filtered) // h
        want = K.filter_types(name.split("-")[1], h)
        assert [filtered[r * rb] for r in range(h)] == want, name


def test_pillow_reads_the_hand_built_files():
    """All five filters cycling, the stream in 1-byte IDAT chunks: Pillow decodes the file to what the unfilter reference gives."""
    for name in ("65x85-cycle-l6", "130x192-cycle-fixed", "2x1-f4-stored", "64x21-f3-l9"):
        h, w, filtered, z = K.grid()[name]
        want = K.unfilter(filtered, h, w)
        assert np.array_equal(K.pillow_decode(K.png_file(h, w, [z], idat_bytes=1)), want), name
        assert np.array_equal(K.pillow_decode(K.png_file(h, w, [z])), want), name
    h, w, filtered, z = K.crafted()["far-distance-32768"]
    assert np.array_equal(K.pillow_decode(K.png_file(h, w, [z])), K.unfilter(filtered, h, w))


def test_filter_rows_and_unfilter_are_inverse():
    img = K.image(65, 21, 2)
    for f in K.FILTERS:
        assert np.array_equal(K.unfilter(K.filter_rows(img, K.filter_types(f, 65)), 65, 21), img), f
    assert np.array_equal(K.unfilter(M.filter_frame(img).tobytes(), 65, 21), img)


# ---- the parser
def test_parser_reads_every_case(tmp_path):
    for name, (h, w, _, z) in K.all_streams().items():
        for step in (None, 1) if len(z) < 3000 else (None,):
            info = D.parse(K.png_file(h, w, [z], idat_bytes=step))
            assert (info.height, info.width, info.n_frames, info.animated) == (h, w, 1, False) and info.frames[0] == z, (name, step)
    img = K.image(33, 50, 1)
    for opt in (False, True):
        info = D.parse(K.pillow_png(img, opt))
        assert (info.height, info.width, info.n_frames) == (33, 50, 1)
        assert np.array_equal(K.unfilter(zlib.decompress(info.frames[0]), 33, 50), img)
    frames = np.stack([K.image(17, 19, i) for i in range(5)])
    streams = M.encode_frames(frames)
    path = P.write_apng(str(tmp_path / "a.png"), streams, 125, 19, 17)
    info = D.parse(open(path, "rb").read())
    assert (info.height, info.width, info.n_frames, info.animated) == (17, 19, 5, True) and info.frames == [bytes(s) for s in streams]
    assert Image.open(path).n_frames == 5
    info = D.parse(open(P.write_apng(str(tmp_path / "one.png"), streams[:1], 125, 19, 17), "rb").read())
    assert info.n_frames == 1 and not info.animated
    # ancillary chunks, a tRNS on colour type 2 among them, are ignored as Pillow ignores them for the pixels of a mode-RGB image
    h, w, filtered, z = K.grid()["2x2-f1-l6"]
    plain = K.png_file(h, w, [z])
    extra = plain[:33] + P._chunk(b"gAMA", struct.pack(">I", 45455)) + P._chunk(b"tRNS", bytes(6)) + P._chunk(b"tEXt", b"k\0v") + plain[33:]
    assert D.parse(extra).frames == [z] and np.array_equal(K.pillow_decode(extra)[..., :3], K.unfilter(filtered, h, w))


def _ihdr(w, h, depth, colour, lace=0):
    return P.SIGNATURE + P._chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour, 0, 0, lace))


def test_parser_refusals(tmp_path):
    def refused(data, word):
        with pytest.raises(D.PngUnsupported, match=word):
            D.parse(data)

    def pil(mode, **kw):
        b = io.BytesIO()
        Image.fromarray(K.image(8, 9, 1)).convert(mode).save(b, format="PNG", **kw)
        return b.getvalue()

    refused(pil("I;16"), "16 bit")
    refused(pil("L"), "greyscale")
    refused(pil("P"), "palette")
    refused(pil("RGBA"), "alpha")
    tail = P._chunk(b"IDAT", zlib.compress(bytes(4))) + P._chunk(b"IEND", b"")
    refused(_ihdr(1, 1, 8, 2, lace=1) + tail, "Adam7")
    refused(_ihdr(65536, 1, 8, 2) + tail, "size")
    refused(_ihdr(8192, 4096, 8, 2) + tail, "size")
    h, w = 17, 19
    streams = M.encode_frames(np.stack([K.image(h, w, i) for i in range(3)]))
    good = open(P.write_apng(str(tmp_path / "a.png"), streams, 100, w, h), "rb").read()
    assert D.parse(good).n_frames == 3

    def chunks(data):
        at, out = 8, []
        while at < len(data):
            n = struct.unpack_from(">I", data, at)[0]
            out.append((data[at + 4:at + 8], data[at + 8:at + 8 + n]))
            at += 12 + n
        return out

    def build(cs):
        return P.SIGNATURE + b"".join(P._chunk(k, b) for k, b in cs)

    cs = chunks(good)
    assert [k for k, _ in cs] == [b"IHDR", b"acTL", b"fcTL", b"IDAT", b"fcTL", b"fdAT", b"fcTL", b"fdAT", b"IEND"]
    part = list(cs)
    part[4] = (b"fcTL", struct.pack(">IIIIIHHBB", 1, w - 1, h, 1, 0, 100, 1000, 0, 0))
    refused(build(part), "partial-frame fcTL")
    # a default image outside the animation: IDAT before the first fcTL (the sequence numbers then start at the next fcTL)
    outside = [cs[0], (b"acTL", struct.pack(">II", 2, 0)), cs[3]]
    seq = 0
    for s in streams[1:]:
        outside.append((b"fcTL", struct.pack(">IIIIIHHBB", seq, w, h, 0, 0, 100, 1000, 0, 0)))
        outside.append((b"fdAT", struct.pack(">I", seq + 1) + s))
        seq += 2
    outside.append(cs[-1])
    assert Image.open(io.BytesIO(build(outside))).n_frames == 3             # (Pillow counts the default image as a frame of its own)
    refused(build(outside), "default image outside the animation")
    assert issubclass(D.PngUnsupported, ValueError)


def test_parser_structural_defects(tmp_path):
    def broken(data, word):
        with pytest.raises(ValueError, match=word) as e:
            D.parse(data)
        assert not isinstance(e.value, D.PngUnsupported), word

    h, w, _, z = K.grid()["65x21-cycle-l6"]
    good = K.png_file(h, w, [z], idat_bytes=100)
    D.parse(good)
    broken(b"\x89PNX" + good[4:], "signature")
    broken(good[:40] + bytes([good[40] ^ 1]) + good[41:], "CRC")
    broken(good[:-1] + b"\x00", "CRC")
    broken(P.SIGNATURE + good[33:], "missing IHDR")
    broken(good[:33] + P._chunk(b"IEND", b""), "missing IDAT")
    for cut in (9, 20, 33, 40, len(good) - 12, len(good) - 1):
        broken(good[:cut], "truncated")
    streams = M.encode_frames(np.stack([K.image(17, 19, i) for i in range(3)]))
    apng = open(P.write_apng(str(tmp_path / "a.png"), streams, 100, 19, 17), "rb").read()
    at = apng.index(b"fdAT")
    swapped = bytearray(apng)
    swapped[at + 4:at + 8] = struct.pack(">I", 7)
    n = struct.unpack_from(">I", apng, at - 4)[0]
    swapped[at + 4 + n:at + 8 + n] = struct.pack(">I", zlib.crc32(bytes(swapped[at:at + 4 + n])) & 0xffffffff)
    broken(bytes(swapped), "sequence")
    last = apng.rindex(b"fcTL") - 4
    broken(apng[:last] + P._chunk(b"IEND", b""), "acTL announces 3 frames")


# ---- the core of the kernels, as a host program under the sanitizers
def test_core_hardening():
    """csrc/pngdec_core.h, the text the kernels compile, with AddressSanitizer and UBSan: every stream of the grid and the crafted ones
    inflates to zlib.decompress's bytes (by one lane and by 64 emulated lanes alike) and unfilters to the reference's rows; the
    documented invalid streams stop with their statuses and positions; 2000 seeded corruptions (byte flips, truncations, splices)
    each end with a status, or with the image zlib itself makes of the stream: no access outside input, output or tables, exit 0."""
    S = K.all_streams()
    assert len(S) == 750 + 13
    status = K.run_host_core([(h, w, z, f, K.unfilter(f, h, w)) for h, w, f, z in S.values()])
    assert not status.any()
    inv = K.invalid_streams()
    got = K.run_host_core([(h, w, z, None, None) for h, w, z, _, _ in inv.values()])
    for (name, (h, w, z, code, where)), (c, p) in zip(inv.items(), got.tolist()):
        assert c == code and (where is None or p == where), (name, c, p)
    assert [v[3] for v in inv.values()] == [2, 11, 8, 9, 10]
    h, w, f, at = K.filter_byte_five()
    assert K.run_host_core([(h, w, None, f, None)]).tolist() == [[12, at]]
    C = K.corruptions()
    assert len(C) == 2000 and {c[0].rsplit("-", 1)[1].rstrip("0123456789") for c in C} == {"flip", "cut", "splice"}
    verdicts = [K.zlib_verdict(z, P.filtered_bytes(h, w)) for _, h, w, z in C]
    got = K.run_host_core([(h, w, z, v, None) for (_, h, w, z), v in zip(C, verdicts)])
    assert set(got[:, 0].tolist()) >= {0, 2, 5, 7, 8, 9, 10, 11}
    assert [int(c) == 0 for c in got[:, 0]] == [v is not None for v in verdicts]


# ---- the C ABI: header, exports and binding agree (the conventions of tests/test_cabi.py)
def test_cabi_pngdec():
    import ctypes
    import re
    from ccedit_amd import hip
    from ccedit_amd.csrc import build as B
    assert "pngdec.hip" in B.SOURCES
    lib = ctypes.CDLL(B.build(force=False, verbose=False))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ccedit_hip.h")).read(), flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(ccedit_[a-z0-9_]+)\s*\(", src)) if n.startswith("ccedit_pngdec_"))
    assert declared == ["ccedit_pngdec_inflate", "ccedit_pngdec_unfilter"]
    for n in declared:
        assert hasattr(lib, n) and n in hip.EXPORTS
        args = re.search(re.escape(n) + r"\s*\(([^)]*)\)", src).group(1)
        assert len(hip._SIGS[n][1]) == len(args.split(",")), n
    assert "#define CCEDIT_ABI_VERSION 12" in src and hip.ABI_VERSION == 12
    l = hip.lib()                                              # argument validation runs before any HIP call
    assert l.ccedit_pngdec_inflate(None, 1, 16, 16, 16, 1, 8, 8, None) == -1 and b"null" in l.ccedit_last_error()
    assert l.ccedit_pngdec_inflate(16, 0, 16, 16, 16, 1, 8, 8, None) == -1 and b"data_bytes" in l.ccedit_last_error()
    assert l.ccedit_pngdec_inflate(16, 1, 12, 16, 16, 1, 8, 8, None) == -1 and b"aligned" in l.ccedit_last_error()
    assert l.ccedit_pngdec_inflate(16, 1, 16, 16, 16, 0, 8, 8, None) == -1 and b"N=0" in l.ccedit_last_error()
    assert l.ccedit_pngdec_inflate(16, 1, 16, 16, 16, 1, 8192, 4096, None) == -1 and b"2^24" in l.ccedit_last_error()
    assert l.ccedit_pngdec_unfilter(16, None, 16, 1, 8, 8, None) == -1 and b"null" in l.ccedit_last_error()
    assert l.ccedit_pngdec_unfilter(16, 16, 18, 1, 8, 8, None) == -1 and b"aligned" in l.ccedit_last_error()
    assert l.ccedit_pngdec_unfilter(16, 16, 16, 1, 0, 8, None) == -1 and l.ccedit_pngdec_unfilter(16, 16, 16, 1, 8, 70000, None) == -1
    assert set(D.STATUS_TEXT) == set(range(1, 13))


# ---- the routing, as far as it goes without a device: what is declined is declined by parsing alone
def test_routing_declines_without_a_device(tmp_path, capsys, monkeypatch):
    from ccedit_amd import video_io as V
    mixed = tmp_path / "mixed"
    mixed.mkdir()
    img = K.image(16, 24, 1)
    Image.fromarray(img).save(str(mixed / "000.png"))
    Image.fromarray(img).save(str(mixed / "001.jpg"))
    paths = [str(mixed / f) for f in sorted(os.listdir(str(mixed)))]
    assert V.files_u8_device((V.PNG,), paths, "cuda", "mixed") is None and V.files_u8_device(V.FILES.device, paths, "cuda", "mixed") is None
    assert capsys.readouterr().err == ""
    odd = tmp_path / "odd"
    odd.mkdir()
    Image.fromarray(img).save(str(odd / "000.png"))
    Image.fromarray(img).convert("RGBA").save(str(odd / "001.png"))
    paths = [str(odd / f) for f in sorted(os.listdir(str(odd)))]
    assert V.files_u8_device((V.PNG,), paths, "cuda", "the clip") is None
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and err.startswith("[pngdec] the clip: 001.png: ") and "alpha" in err
    assert err.endswith("this clip is decoded by Pillow on the host\n")
    bad = tmp_path / "bad.png"
    data = open(str(odd / "000.png"), "rb").read()
    bad.write_bytes(data[:50] + bytes([data[50] ^ 4]) + data[51:])
    assert V.files_u8_device((V.PNG,), [str(bad)], "cuda", "one") is None and "CRC" in capsys.readouterr().err
    assert V.files_u8_device((V.PNG,), [], "cuda", "none") is None
    # a status from the device names file, frame, code and byte position (the decoder itself is stood in for: there is no device here)
    Image.fromarray(img[::-1]).save(str(odd / "001.png"))
    Image.fromarray(img[:8]).save(str(odd / "002.png"))

    def stopped(datas, device, infos=None):
        if datas[-1] == open(paths[1], "rb").read():
            raise ValueError(f"frame {len(datas) - 1}: Adler-32 mismatch (code 11 at byte 77)")
        return None
    monkeypatch.setattr(D, "decode", stopped)
    with pytest.raises(ValueError, match=r"^the clip: 001.png: frame 1: Adler-32 mismatch \(code 11 at byte 77\)$"):
        V.files_u8_device((V.PNG,), paths, "cuda", "the clip")                       # same size: one call
    with pytest.raises(ValueError, match=r"^the clip: 001.png: frame 1: Adler-32 mismatch \(code 11 at byte 77\)$"):
        V.files_u8_device((V.PNG,), paths + [str(odd / "002.png")], "cuda", "the clip")      # another size among them: a call per file
    monkeypatch.undo()
    anim = P.write_apng(str(tmp_path / "rgba.png"), M.encode_frames(np.stack([K.image(8, 9, i) for i in range(2)])), 100, 9, 8)
    raw = bytearray(open(anim, "rb").read())
    at = raw.rindex(b"fcTL")
    raw[at + 8:at + 12] = struct.pack(">I", 8)                                   # a narrower second frame
    raw[at + 30:at + 34] = struct.pack(">I", zlib.crc32(bytes(raw[at:at + 30])) & 0xffffffff)
    open(anim, "wb").write(bytes(raw))
    assert V.clip_u8_device(V.APNG.device, anim, "cuda") is None
    err = capsys.readouterr().err
    assert err.startswith("[pngdec] ") and "partial-frame fcTL" in err and err.endswith("this clip is decoded by Pillow on the host\n")
