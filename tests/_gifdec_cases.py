"""Inputs shared by tests/test_gifdec.py (the parser, the numpy restatement and the host build of csrc/gifdec_core.h) and
tests/test_gifdec_gpu.py (the kernels): a small GIF writer whose LZW encoder has switches (minimum code size, Clear policy, EOI, surplus
bytes) and whose frame descriptors are free, the cases built with it — the smallest shapes at which each mechanism can go wrong —, files
from the project's own two GIF writers, seeded corruptions, and the bridge to the stand-alone host program (tests/gifdec_harden.cpp).
The references are Pillow for whole files (video_io._sequence_u8) and tests/_gifdec_numpy.py for the stages.  Everything is computed
once per process and never changed."""
from __future__ import annotations

import functools
import os
import shutil
import struct
import subprocess
import tempfile

import numpy as np

import _gifdec_numpy as R
from _gif_cases import content

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ---- the LZW encoder, with switches
def lzw_encode(indices, m=8, start_clear=True, policy="deferred", eoi=True, surplus=b"", clear_before=()):
    """Indices in stream order -> the LZW byte stream.  policy: "full" (a Clear when the table is full), "deferred" (none: the full
    table stays), ("every", k) (a Clear after every k data codes).  clear_before: data-code counts before which a Clear is put (a count
    given twice: two Clears in a row)."""
    idx = [int(v) for v in np.asarray(indices).reshape(-1)]
    assert all(0 <= v < (1 << m) for v in idx)
    clear, emax = 1 << m, 4096 - ((1 << m) + 2)
    acc = nbits = 0
    j = total = 0                                  # data codes since the last Clear, and in all
    table = {}
    pending = sorted(clear_before)

    def put(code):
        nonlocal acc, nbits
        acc |= code << nbits
        nbits += R.width_at(m, j)

    def put_clear():
        nonlocal j
        put(clear)
        j = 0
        table.clear()

    if start_clear:
        put_clear()
    i, n = 0, len(idx)
    while i < n:
        while pending and pending[0] <= total:
            pending.pop(0)
            put_clear()
        code, length = idx[i], 1
        while i + length < n and (code, idx[i + length]) in table:
            code = table[(code, idx[i + length])]
            length += 1
        put(code)
        if i + length < n and j < emax:
            table[(code, idx[i + length])] = clear + 2 + j
        j += 1
        total += 1
        i += length
        if i < n and ((policy == "full" and j >= emax) or (isinstance(policy, tuple) and j >= policy[1])):
            put_clear()
    if eoi:
        put(clear + 1)
    return acc.to_bytes((nbits + 7) // 8, "little") + bytes(surplus)


def count_codes(stream, m, npix):
    return len(R.code_table(stream, m, npix)[0])


# ---- the container
def palette_of(n, seed=0):
    return np.random.RandomState(100 + seed).randint(0, 256, size=(n, 3)).astype(np.uint8).tobytes()


def frame(indices, x=0, y=0, interlace=False, disposal=0, transparent=None, palette=None, m=8, stream=None, **lzw):
    """One frame: indices (h, w) in display order (rows go out in four-pass order when interlaced); stream: given instead of encoded."""
    a = np.asarray(indices)
    h, w = a.shape
    rows = a[R.interlaced_rows(h)] if interlace else a
    return dict(x=x, y=y, w=w, h=h, interlace=interlace, disposal=disposal, transparent=transparent, palette=palette, m=m,
                stream=lzw_encode(rows, m, **lzw) if stream is None else stream)


def _table_bits(palette):
    n = len(palette) // 3
    assert n in (2, 4, 8, 16, 32, 64, 128, 256) and len(palette) == 3 * n
    return n.bit_length() - 2


def gif_file(width, height, frames, global_palette=None, trailer=True) -> bytes:
    out = [b"GIF89a", struct.pack("<HHBBB", width, height, (0x80 | _table_bits(global_palette)) if global_palette else 0, 0, 0)]
    if global_palette:
        out.append(global_palette)
    for f in frames:
        t = f["transparent"]
        out.append(bytes([0x21, 0xF9, 4, f["disposal"] << 2 | (t is not None), 10, 0, t or 0, 0]))
        out.append(bytes([0x21, 0xFE, 3]) + b"abc" + b"\x00")                                   # (a comment extension: skipped by its sub-blocks)
        pal = f["palette"]
        out.append(bytes([0x2C]) + struct.pack("<HHHHB", f["x"], f["y"], f["w"], f["h"],
                                               (0x80 | _table_bits(pal) if pal else 0) | (0x40 if f["interlace"] else 0)))
        if pal:
            out.append(pal)
        out.append(bytes([f["m"]]))
        s = f["stream"]
        out.extend(bytes([len(s[at:at + 255])]) + s[at:at + 255] for at in range(0, len(s), 255))
        out.append(b"\x00")
    if trailer:
        out.append(b"\x3b")
    return b"".join(out)


def noise(h, w, colours, seed):
    return np.random.RandomState(seed).randint(0, colours, size=(h, w)).astype(np.uint8)


def _quantised(img, palette):
    """Photo-like indices: the nearest of the palette's first entries by luminance rank (any index field will do: it is a test input)."""
    n = len(palette) // 3
    lum = img.astype(np.int32).sum(-1)
    return (lum * n // (3 * 255 + 1)).astype(np.uint8)


# ---- the served cases: name -> the file's bytes
@functools.lru_cache(maxsize=None)
def served():
    out = {}
    g256 = palette_of(256)
    # code sizes and widths
    for m in range(2, 9):
        pal = palette_of(1 << m, m)
        out[f"m{m}-noise"] = gif_file(50, 40, [frame(noise(40, 50, 1 << m, m), m=m)], pal)
        out[f"m{m}-photo"] = gif_file(50, 40, [frame(_quantised(content("photo", 40, 50, m), pal), m=m, policy="full")], pal)
    big = noise(64, 96, 256, 1)
    out["noise-deferred-clear"] = gif_file(96, 64, [frame(big, policy="deferred")], g256)          # widths 9 -> 12, the table fills and stays full
    out["noise-clear-at-full"] = gif_file(96, 64, [frame(big, policy="full")], g256)
    out["noise-m2-table-fills"] = gif_file(192, 128, [frame(noise(128, 192, 4, 2), m=2, policy="deferred")], palette_of(4))
    # KwKwK and long chains
    out["flat-48x72"] = gif_file(72, 48, [frame(np.full((48, 72), 7, np.uint8))], g256)
    out["flat-256x256"] = gif_file(256, 256, [frame(np.full((256, 256), 200, np.uint8))], g256)
    out["stripes"] = gif_file(72, 48, [frame(np.tile(np.array([3, 9], np.uint8), (48, 36)))], g256)
    # batch edges: 100 pixels whose pairs never repeat -> one code per pixel
    ramp = np.arange(100, dtype=np.uint8)[None]
    for at in (0, 1, 63, 64):
        out[f"clear-as-code-{at}"] = gif_file(100, 1, [frame(ramp, start_clear=False, clear_before=(at,))], g256)
    out["eoi-as-64th-code"] = gif_file(63, 1, [frame(ramp[:, :63], start_clear=False)], g256)
    for n in (1, 2, 63, 64, 65):
        out[f"codes-{n}"] = gif_file(n, 1, [frame(ramp[:, :n], start_clear=False, eoi=False)], g256)
    out["1x1"] = gif_file(1, 1, [frame(np.array([[5]], np.uint8))], g256)
    out["two-clears-in-a-row"] = gif_file(100, 1, [frame(ramp, clear_before=(30, 30))], g256)
    out["no-clear-at-the-start"] = gif_file(50, 40, [frame(noise(40, 50, 256, 3), start_clear=False)], g256)
    out["clear-every-37-codes"] = gif_file(50, 40, [frame(noise(40, 50, 16, 4), policy=("every", 37))], g256)
    out["no-eoi-and-surplus"] = gif_file(50, 40, [frame(noise(40, 50, 64, 5), eoi=False, surplus=b"\x55\xaa\x00\xff" * 5)], g256)
    # sub-blocks: streams of 254, 255, 256 and 510 bytes (a noise frame of 16 x 14 takes 254 bytes; surplus bytes fill up)
    small = noise(14, 16, 256, 6)
    base = lzw_encode(small)
    assert len(base) <= 254, len(base)
    for n in (254, 255, 256, 510):
        out[f"stream-{n}-bytes"] = gif_file(16, 14, [frame(small, stream=base + bytes(1 + i % 255 for i in range(n - len(base))))], g256)
    # frames
    first = frame(noise(30, 40, 256, 7))
    corners = [frame(noise(7, 5, 256, 8 + i), x=x, y=y) for i, (x, y) in enumerate(((0, 0), (35, 0), (0, 23), (35, 23)))]
    out["rectangles-at-the-corners"] = gif_file(40, 30, [first] + corners + [frame(np.array([[9]], np.uint8), x=17, y=11)], g256)
    for h in (1, 2, 3, 4, 5, 8, 9):
        out[f"interlaced-{h}-rows"] = gif_file(12, 9, [frame(noise(9, 12, 256, 20)), frame(noise(h, 7, 256, 21 + h), x=2, y=0, interlace=True)], g256)
    out["interlaced-first-frame"] = gif_file(16, 13, [frame(noise(13, 16, 256, 31), interlace=True), frame(noise(13, 16, 256, 32), interlace=True)], g256)
    l16 = palette_of(16, 40)
    out["transparent-local-palette"] = gif_file(40, 30, [first, frame(noise(20, 25, 16, 41), x=3, y=4, transparent=5, palette=l16, m=4),
                                                          frame(noise(30, 40, 16, 42), transparent=0, palette=l16, m=4)], g256)
    out["transparent-global-palette"] = gif_file(40, 30, [first, frame(noise(20, 25, 8, 43), x=10, y=9, transparent=3, m=3),
                                                           frame(noise(11, 13, 256, 44), x=1, y=2, transparent=255)], g256)
    out["short-palettes"] = gif_file(40, 30, [frame(noise(30, 40, 4, 45), m=2), frame(noise(9, 9, 16, 46), x=5, y=5, palette=l16, m=4),
                                                frame(noise(9, 9, 2, 47), x=20, y=5, palette=palette_of(2, 48), m=2)], palette_of(4, 49))
    out["disposal-1"] = gif_file(40, 30, [dict(first, disposal=1), frame(noise(8, 8, 256, 50), x=4, y=4, disposal=1, transparent=1),
                                            frame(noise(8, 8, 256, 51), x=20, y=10, disposal=1)], g256)
    out["disposal-2-on-the-last-frame"] = gif_file(40, 30, [first, frame(noise(8, 8, 256, 52), x=4, y=4, disposal=2, transparent=2)], g256)
    out["local-palettes-only"] = gif_file(40, 30, [dict(first, palette=palette_of(256, 53)), frame(noise(8, 8, 16, 54), x=1, y=1, palette=l16, m=4)])
    return out


@functools.lru_cache(maxsize=None)
def writer_clips():
    """Photo-like frames through the project's two GIF writers: name -> the file's bytes."""
    import _gif_numpy as G
    from ccedit_amd import video_io
    frames = np.stack([content("photo", 48, 65, s) for s in range(3)])                    # 3120 pixels: one chunk of 3072 and a tail
    work = tempfile.mkdtemp(prefix="gifdec_clips_")
    path = video_io._write_gif_pillow(os.path.join(work, "pillow.gif"), list(frames), 10)
    with open(path, "rb") as f:
        pillow = f.read()
    shutil.rmtree(work, ignore_errors=True)
    return {"pillow-writer": pillow, "device-writer-format": G.file_bytes(G.encode_frames(frames), 100, 65, 48)}


def all_served():
    d = dict(served())
    d.update(writer_clips())
    return d


# ---- declined by the parser: name -> (the file's bytes, a piece of the reason)
@functools.lru_cache(maxsize=None)
def declined():
    g = palette_of(256)
    full, part = frame(noise(30, 40, 256, 60)), frame(noise(8, 8, 256, 61), x=4, y=4)
    good = gif_file(40, 30, [full, part], g)
    return {"frame-0-partial": (gif_file(40, 30, [part, full], g), "a partial first frame"),
            "frame-0-transparent": (gif_file(40, 30, [dict(full, transparent=4), part], g), "a transparent first frame"),
            "disposal-2-in-mid-clip": (gif_file(40, 30, [full, dict(part, disposal=2), part], g), "disposal 2 before the last frame"),
            "disposal-3-in-mid-clip": (gif_file(40, 30, [full, dict(part, disposal=3), part], g), "disposal 3 before the last frame"),
            "rectangle-outside-the-canvas": (gif_file(40, 30, [full, dict(part, x=36)], g), "outside the canvas"),
            "no-palette": (gif_file(40, 30, [full, part]), "no palette"),
            "min-code-size-1": (gif_file(40, 30, [full, dict(part, m=1)], g), "minimum code size 1"),
            "min-code-size-9": (gif_file(40, 30, [full, dict(part, m=9)], g), "minimum code size 9"),
            "truncated-container": (good[:-1], "truncated file")}


# ---- stopped on the device: name -> (the file's bytes, status, the frame it names)
def _codes(values, m=8):
    """Raw code values -> a stream, widths as a decoder expects them (Clear resets the count)."""
    acc = nbits = j = 0
    for v in values:
        w = R.width_at(m, j)
        acc |= v << nbits
        nbits += w
        j = 0 if v == 1 << m else j + 1
    return acc.to_bytes((nbits + 7) // 8, "little")


@functools.lru_cache(maxsize=None)
def stopped():
    g = palette_of(256)
    full, idx = frame(noise(30, 40, 256, 70)), noise(8, 8, 256, 71)
    good = lzw_encode(idx)

    def two(second):
        return gif_file(40, 30, [full, dict(frame(idx, x=4, y=4), **second)], g)

    return {"code-above-the-next-free-entry": (two(dict(stream=_codes([256, 5, 6, 300, 7]))), R.CODE_ABOVE_NEXT, 1),
            "non-literal-after-clear": (two(dict(stream=_codes([256, 5, 6, 256, 258]))), R.FIRST_NOT_LITERAL, 1),
            "stream-cut-short": (two(dict(stream=good[:len(good) // 2])), R.STREAM_SHORT, 1),
            "eoi-before-the-last-pixel": (two(dict(stream=_codes([256, 5, 6, 7, 257]))), R.STREAM_SHORT, 1),
            "index-beyond-the-palette": (two(dict(stream=lzw_encode(noise(8, 8, 16, 72) | 8, 4), m=4, palette=palette_of(4, 73))), R.BAD_INDEX, 1)}


# ---- the streams of every case: (name, m, npix, stream)
@functools.lru_cache(maxsize=None)
def case_streams():
    from ccedit_amd import gifdec
    out = []
    for group in (all_served(), {k: v[0] for k, v in stopped().items()}):
        for name, data in group.items():
            for i, f in enumerate(gifdec.parse(data).frames):
                out.append((f"{name}/{i}", f.min_code, f.w * f.h, f.stream))
    return out


# ---- 2000 seeded corruptions of the valid streams: (name, m, npix, bytes)
@functools.lru_cache(maxsize=None)
def corruptions(n: int = 2000):
    rs = np.random.RandomState(13)
    pool = [c for c in case_streams() if 2 <= len(c[3]) <= 4096]
    out = []
    for i in range(n):
        name, m, npix, z = pool[rs.randint(len(pool))]
        z = bytearray(z)
        how = ("flip", "cut", "splice")[i % 3]
        at = int(rs.randint(len(z)))
        if how == "flip":
            z[at] ^= 1 << int(rs.randint(8))
        elif how == "cut":
            del z[at:]
        else:
            other = pool[rs.randint(len(pool))][3]
            frm = int(rs.randint(len(other)))
            z[at:] = other[frm:frm + int(rs.randint(1, 64))] + bytes(z[at + int(rs.randint(0, 8)):])
        out.append((f"{name}-{how}{i}", m, npix, bytes(z)))
    return out


# ---- the host program (tests/gifdec_harden.cpp): gifdec_core.h under the host's sanitizers
@functools.lru_cache(maxsize=None)
def harden_exe() -> str:
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(tempfile.mkdtemp(prefix="gifdec_harden_"), "gifdec_harden")
    clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libsan" if clang else "-static-libasan"]
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", *san, os.path.join(ROOT, "tests", "gifdec_harden.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    return exe


def run_host_core(cases):
    """cases: (m, npix, stream, indices or None).  Every stream is decoded by one lane and by 64 emulated lanes; the program compares
    the two and, where indices are given, the decoded indices with them (None: any defined status will do).  -> int64 (n, 3): status,
    bit position and number of codes of every case, after the program ended with exit status 0, no mismatch and nothing on stderr."""
    work = tempfile.mkdtemp(prefix="gifdec_cases_")
    path, res = os.path.join(work, "cases.bin"), os.path.join(work, "result.txt")
    with open(path, "wb") as f:
        f.write(b"GDH1" + struct.pack("<i", len(cases)))
        for m, npix, stream, indices in cases:
            f.write(struct.pack("<iqqi", m, npix, len(stream), int(indices is not None)))
            f.write(stream)
            if indices is not None:
                assert len(indices) == npix
                f.write(bytes(indices))
    run = subprocess.run([harden_exe(), path, res], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr.strip(), (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    assert f"{len(cases)} cases" in run.stdout and " 0 mismatches" in run.stdout, run.stdout
    out = np.loadtxt(res, dtype=np.int64, ndmin=2)
    shutil.rmtree(work, ignore_errors=True)
    assert out.shape == (len(cases), 3)
    return out


# ---- the references of every served case, computed once: Pillow's frames, and per frame the reference's table and indices
def pillow_frames(data: bytes) -> np.ndarray:
    """The file as the host route decodes it (video_io._sequence_u8: Pillow)."""
    from ccedit_amd import video_io
    work = tempfile.mkdtemp(prefix="gifdec_pillow_")
    path = os.path.join(work, "clip.gif")
    with open(path, "wb") as f:
        f.write(data)
    out = video_io._sequence_u8(path)
    shutil.rmtree(work, ignore_errors=True)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(name: str):
    """-> (parsed file, Pillow's frames, per frame (parent, length, first, last, off), per frame the indices in stream order)"""
    from ccedit_amd import gifdec
    data = all_served()[name]
    info = gifdec.parse(data)
    tables, planes = [], []
    for f in info.frames:
        t = R.code_table(f.stream, f.min_code, f.w * f.h)
        assert t[5] == R.OK, (name, t[5:])
        tables.append(t[:5])
        planes.append(R.code_pixels(t[0], t[1], t[3], t[4], f.w * f.h))
    return info, pillow_frames(data), tables, planes
