"""Inputs shared by tests/test_pngdec.py (the parser and the host build of csrc/pngdec_core.h) and tests/test_pngdec_gpu.py (the kernels):
PNGs assembled by hand over a grid of filters, stream kinds and sizes, crafted deflate streams, seeded corruptions, and the bridge to
the stand-alone host program (tests/pngdec_harden.cpp).  The references are zlib.decompress for the inflate stage, the numpy unfilter
below for the unfilter stage and Pillow for whole files.  Everything is computed once per process and never changed."""
from __future__ import annotations

import functools
import io
import os
import shutil
import struct
import subprocess
import tempfile
import zlib

import numpy as np

from _gif_cases import content
from ccedit_amd import png as P

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
WIDTHS = (1, 2, 21, 85, 192)          # row bytes 4, 7, 64, 256, 577: on and across the 64- and 256-byte lane boundaries
HEIGHTS = (1, 2, 64, 65, 130)         # one more row than a wave, and two wraps
FILTERS = ("f0", "f1", "f2", "f3", "f4", "cycle")
KINDS = ("stored", "fixed", "l1", "l6", "l9")
CONTENTS = ("photo", "noise", "ramp", "checker")


# ---- the filters, forwards (to assemble files) and backwards (the reference of the unfilter stage)
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(img: np.ndarray, types) -> bytes:
    """uint8 (H, W, 3) -> the filtered bytes H * (1 + 3 W), row r filtered with types[r]."""
    h, w, _ = img.shape
    x = img.reshape(h, 3 * w).astype(np.int32)
    out = np.zeros((h, 1 + 3 * w), np.uint8)
    for r in range(h):
        a = np.concatenate([np.zeros(3, np.int32), x[r, :-3]])
        b = x[r - 1] if r else np.zeros(3 * w, np.int32)
        c = np.concatenate([np.zeros(3, np.int32), b[:-3]])
        pred = (np.zeros_like(a), a, b, (a + b) >> 1, _paeth(a, b, c))[types[r]]
        out[r, 0] = types[r]
        out[r, 1:] = (x[r] - pred) & 255
    return out.tobytes()


def unfilter(filtered: bytes, h: int, w: int) -> np.ndarray:
    """The reference of the unfilter stage: bytes H * (1 + 3 W) with filter bytes 0 ... 4 -> uint8 (H, W, 3)."""
    return _unfilter(bytes(filtered), h, w)


@functools.lru_cache(maxsize=None)
def _unfilter(filtered: bytes, h: int, w: int) -> np.ndarray:
    rb, up, rows = 1 + 3 * w, bytes(3 * w + 3), []                  # (a zero row above, a zero pixel to the left; plain ints: the walk is serial)
    for r in range(h):
        ft, x, cur = filtered[r * rb], filtered[r * rb + 1:(r + 1) * rb], bytearray(3 * w + 3)
        for i in range(3, 3 * w + 3):
            a, b, c = cur[i - 3], up[i], up[i - 3]
            p = a + b - c
            pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
            pred = (0, a, b, (a + b) >> 1, a if pa <= pb and pa <= pc else (b if pb <= pc else c))[ft]
            cur[i] = (x[i - 3] + pred) & 255
        rows.append(bytes(cur[3:]))
        up = cur
    out = np.frombuffer(b"".join(rows), np.uint8).reshape(h, w, 3)
    out.setflags(write=False)
    return out


def filter_types(name: str, h: int):
    return [r % 5 for r in range(h)] if name == "cycle" else [int(name[1])] * h


# ---- zlib streams of every kind
def compress(data: bytes, kind: str) -> bytes:
    if kind == "stored":
        co = zlib.compressobj(0)
    elif kind == "fixed":
        co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
    else:
        co = zlib.compressobj(int(kind[1]))
    return co.compress(data) + co.flush()


class Bits:
    """LSB-first bit writer; Huffman codes go in MSB first."""
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value: int, bits: int):
        self.acc |= value << self.n
        self.n += bits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code: int, bits: int):
        self.put(int(format(code, f"0{bits}b")[::-1], 2), bits)

    def done(self) -> bytes:
        if self.n:
            self.put(0, 8 - self.n)
        return bytes(self.out)


def _fixed_litlen(b: Bits, s: int):
    if s < 144:
        b.code(0x30 + s, 8)
    elif s < 256:
        b.code(0x190 + s - 144, 9)
    elif s < 280:
        b.code(s - 256, 7)
    else:
        b.code(0xC0 + s - 280, 8)


def fixed_block(b: Bits, tokens, final: bool, raw_dist_code=None):
    """One fixed-Huffman block: tokens are literals (int) or matches (length, distance)."""
    b.put(1 if final else 0, 1)
    b.put(1, 2)
    for t in tokens:
        if isinstance(t, int):
            _fixed_litlen(b, t)
            continue
        length, dist = t
        k = max(i for i in range(29) if P.LEN_BASE[i] <= length) if length < 258 else 28
        _fixed_litlen(b, 257 + k)
        b.put(length - P.LEN_BASE[k], P.LEN_EXTRA[k])
        if raw_dist_code is not None:
            b.code(raw_dist_code, 5)
            continue
        k = max(i for i in range(30) if P.DIST_BASE[i] <= dist)
        b.code(k, 5)
        b.put(dist - P.DIST_BASE[k], P.DIST_EXTRA[k])
    _fixed_litlen(b, 256)


def zwrap(deflate: bytes, data: bytes, adler=None) -> bytes:
    return b"\x78\x9c" + deflate + struct.pack(">I", (zlib.adler32(data) if adler is None else adler) & 0xffffffff)


def mixed_blocks(data: bytes) -> bytes:
    """A zlib stream of blocks of all three kinds: thirds of `data` through three raw deflate coders (stored, fixed, dynamic), the first
    two ended with a sync flush (an empty stored block, byte aligned), so the pieces concatenate."""
    n = len(data) // 3
    parts = []
    for piece, (level, strategy), last in ((data[:n], (0, zlib.Z_DEFAULT_STRATEGY), False), (data[n:2 * n], (6, zlib.Z_FIXED), False),
                                           (data[2 * n:], (9, zlib.Z_DEFAULT_STRATEGY), True)):
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        parts.append(co.compress(piece) + co.flush(zlib.Z_FINISH if last else zlib.Z_SYNC_FLUSH))
    return zwrap(b"".join(parts), data)


# ---- the container
def png_file(h: int, w: int, streams, idat_bytes=None, duration_ms=100) -> bytes:
    """A PNG (one stream) or APNG (several) of 8-bit RGB around the given zlib streams; idat_bytes: the first stream cut into IDAT chunks
    of that many bytes."""
    parts = [P.SIGNATURE, P._chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))]
    seq = 0
    if len(streams) > 1:
        parts.append(P._chunk(b"acTL", struct.pack(">II", len(streams), 0)))
    for i, s in enumerate(streams):
        if len(streams) > 1:
            parts.append(P._chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, w, h, 0, 0, duration_ms, 1000, 0, 0)))
            seq += 1
        if i == 0:
            step = idat_bytes or max(len(s), 1)
            parts.extend(P._chunk(b"IDAT", s[at:at + step]) for at in range(0, len(s), step))
        else:
            parts.append(P._chunk(b"fdAT", struct.pack(">I", seq) + s))
            seq += 1
    parts.append(P._chunk(b"IEND", b""))
    return b"".join(parts)


def pillow_decode(data: bytes) -> np.ndarray:
    from PIL import Image
    return np.array(Image.open(io.BytesIO(data)))


def pillow_png(img: np.ndarray, optimize: bool) -> bytes:
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="PNG", optimize=optimize)
    return b.getvalue()


def image(h: int, w: int, seed: int) -> np.ndarray:
    return np.ascontiguousarray(content(CONTENTS[seed % len(CONTENTS)], h, w, seed))


# ---- the grid: name -> (h, w, filtered bytes, zlib stream)
@functools.lru_cache(maxsize=None)
def grid():
    out = {}
    seed = 0
    for h in HEIGHTS:
        for w in WIDTHS:
            for f in FILTERS:
                seed += 1
                filtered = filter_rows(image(h, w, seed), filter_types(f, h))
                for kind in KINDS:
                    out[f"{h}x{w}-{f}-{kind}"] = (h, w, filtered, compress(filtered, kind))
    return out


@functools.lru_cache(maxsize=None)
def crafted():
    """The stream kinds zlib's coder does not write on its own, and the other sources.  name -> (h, w, filtered bytes, zlib stream)."""
    import _png_numpy as M
    out = {}
    h, w = 130, 192                                                  # 75 010 filtered bytes: more than 64 KiB
    noise = filter_rows(content("noise", h, w, 5), filter_types("cycle", h))
    out["noise-mixed-blocks"] = (h, w, noise, mixed_blocks(noise))
    out["noise-l6-several-blocks"] = (h, w, noise, compress(noise, "l6"))
    zeros = bytes(P.filtered_bytes(65, 85))
    out["zeros-l9-overlapping-copies"] = (65, 85, zeros, compress(zeros, "l9"))
    # rows of 4096 bytes (W = 1365): row 8 repeats row 0 at distance 32768, which zlib's coder never reaches (its window stops 262 short)
    h, w = 9, 1365
    rows = bytearray(filter_rows(content("noise", 8, w, 9), filter_types("cycle", 8)))
    far = bytes(rows) + bytes(rows[:4096])
    b = Bits()
    fixed_block(b, list(rows) + [(258, 32768)] * 15 + [(226, 32768)], True)
    assert 15 * 258 + 226 == 4096 and P.filtered_bytes(h, w) == len(far)
    out["far-distance-32768"] = (h, w, far, zwrap(b.done(), far))
    for i, (hh, ww) in enumerate(((17, 19), (64, 85), (65, 192))):
        img = image(hh, ww, 40 + i)
        own = M.filter_frame(img).tobytes()
        out[f"own-encoder-{hh}x{ww}"] = (hh, ww, own, M.zlib_stream(own))
        for opt in (False, True):
            info = _parse(pillow_png(img, opt))
            out[f"pillow-{'opt' if opt else 'std'}-{hh}x{ww}"] = (hh, ww, zlib.decompress(info.frames[0]), info.frames[0])
    return out


def _parse(data):
    from ccedit_amd import pngdec
    return pngdec.parse(data)


def all_streams():
    d = dict(grid())
    d.update(crafted())
    return d


# ---- invalid streams with documented statuses: name -> (h, w, zlib stream, code, position or None)
@functools.lru_cache(maxsize=None)
def invalid_streams():
    h, w = 17, 19
    good = grid()[f"64x85-cycle-l6"]
    gh, gw, gdata, gz = good
    out = {"cut-in-the-middle": (gh, gw, gz[:len(gz) // 2], 2, len(gz) // 2),
           "wrong-adler": (gh, gw, gz[:-4] + struct.pack(">I", (zlib.adler32(gdata) + 1) & 0xffffffff), 11, len(gz) - 4)}
    data = bytes(range(58)) * h
    assert len(data) == P.filtered_bytes(h, w)
    b = Bits()
    fixed_block(b, list(data[:10]) + [(20, 11)], True)                 # ten bytes out, then a match eleven back
    out["distance-before-the-start"] = (h, w, zwrap(b.done(), data), 8, None)
    for name, extra, code in (("output-one-byte-long", 1, 9), ("output-one-byte-short", -1, 10)):
        body = data + b"\x07" if extra > 0 else data[:-1]
        out[name] = (h, w, compress(body, "l6"), code, None)
    return out


def filter_byte_five():
    """-> (h, w, filtered bytes whose row 70 has filter byte 5, that byte's offset)"""
    h, w = 130, 21
    f = bytearray(filter_rows(image(h, w, 3), filter_types("cycle", h)))
    f[70 * (1 + 3 * w)] = 5
    return h, w, bytes(f), 70 * (1 + 3 * w)


# ---- 2000 seeded corruptions of small streams: (name, h, w, bytes)
@functools.lru_cache(maxsize=None)
def corruptions(n: int = 2000):
    rs = np.random.RandomState(11)
    pool = [(k, v) for k, v in all_streams().items() if len(v[3]) <= 4096]
    out = []
    for i in range(n):
        name, (h, w, _, z) = pool[rs.randint(len(pool))]
        z = bytearray(z)
        how = ("flip", "cut", "splice")[i % 3]
        at = int(rs.randint(len(z)))
        if how == "flip":
            z[at] ^= 1 << int(rs.randint(8))
        elif how == "cut":
            del z[at:]
        else:
            _, (_, _, _, other) = pool[rs.randint(len(pool))]
            frm = int(rs.randint(len(other)))
            z[at:] = other[frm:frm + int(rs.randint(1, 64))] + bytes(z[at + int(rs.randint(0, 8)):])
        out.append((f"{name}-{how}{i}", h, w, bytes(z)))
    return out


def zlib_verdict(z: bytes, length: int):
    """What zlib makes of the stream: its output when it accepts the stream AND the output has the expected length, else None."""
    try:
        d = zlib.decompress(z)
    except zlib.error:
        return None
    return d if len(d) == length else None


# ---- the host program (tests/pngdec_harden.cpp): pngdec_core.h under the host's sanitizers
@functools.lru_cache(maxsize=None)
def harden_exe() -> str:
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(tempfile.mkdtemp(prefix="pngdec_harden_"), "pngdec_harden")
    clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libsan" if clang else "-static-libasan"]
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", *san, os.path.join(ROOT, "tests", "pngdec_harden.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    return exe


def run_host_core(cases):
    """cases: (h, w, zlib stream or None, filtered bytes or None, rgb or None).  With a stream: inflate (then, on status 0, unfilter);
    without: unfilter of the given filtered bytes.  filtered / rgb, where given, are what the program must reproduce; filtered = None
    with a stream: the stream must stop with a status.  -> int32 (n, 2): status and position of every case, after the program ended
    with exit status 0, no mismatch and nothing on stderr (no sanitizer report)."""
    work = tempfile.mkdtemp(prefix="pngdec_cases_")
    path, res = os.path.join(work, "cases.bin"), os.path.join(work, "result.txt")
    with open(path, "wb") as f:
        f.write(b"PDH1" + struct.pack("<i", len(cases)))
        for h, w, z, filtered, rgb in cases:
            f.write(struct.pack("<iiqii", h, w, -1 if z is None else len(z), int(filtered is not None), int(rgb is not None)))
            f.write(z or b"")
            if filtered is not None:
                assert len(filtered) == P.filtered_bytes(h, w)
                f.write(filtered)
            if rgb is not None:
                f.write(np.ascontiguousarray(rgb, np.uint8).tobytes())
    run = subprocess.run([harden_exe(), path, res], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr.strip(), (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    assert f"{len(cases)} cases" in run.stdout and " 0 mismatches" in run.stdout, run.stdout
    out = np.loadtxt(res, dtype=np.int64, ndmin=2).astype(np.int32)
    shutil.rmtree(work, ignore_errors=True)
    assert out.shape == (len(cases), 2)
    return out
