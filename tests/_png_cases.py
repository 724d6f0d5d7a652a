"""Inputs shared by tests/test_png.py (the numpy restatement against zlib and Pillow) and tests/test_png_gpu.py (the kernels against the
restatement): frame shapes, crafted byte streams for the deflate stages, crafted histograms for the code construction.  References are
computed once per process and never changed."""
from __future__ import annotations

import functools

import numpy as np

import _png_numpy as M
from _gif_cases import content
from ccedit_amd import png as P

CONTENTS = ["flat", "ramp", "checker", "photo", "noise"]
SMALL_SHAPES = [(1, 1), (1, 7), (7, 1), (17, 19), (33, 50), (64, 96)]
# H * (1 + 3 W) = CHUNK - 1, CHUNK, CHUNK + 1, 2 CHUNK + 1: CHUNK is no multiple of the row, so the chunk borders fall inside rows
BORDER_SHAPES = {P.CHUNK - 1: (129, 42), P.CHUNK: (64, 85), P.CHUNK + 1: (113, 48), 2 * P.CHUNK + 1: (99, 110)}
assert all(P.filtered_bytes(h, w) == n for n, (h, w) in BORDER_SHAPES.items())


def frame(kind: str, h: int, w: int, seed: int = 0) -> np.ndarray:
    return np.ascontiguousarray(content(kind, h, w, seed))


@functools.lru_cache(maxsize=None)
def clip(h: int, w: int, n: int = 3) -> np.ndarray:
    """n frames cycling through CONTENTS, uint8 (n, h, w, 3)."""
    return np.stack([frame(CONTENTS[i % len(CONTENTS)], h, w, i) for i in range(n)], axis=0)


def _period(d: int, base: int, reps: int = 12) -> bytes:
    """d fresh byte values, then the same d bytes again and again: a match at distance d."""
    return bytes(range(base, base + d)) * reps


@functools.lru_cache(maxsize=None)
def streams():
    """name -> bytes: what the token stage is fed directly."""
    rs = np.random.RandomState(7)
    far = bytearray(P.CHUNK)
    far[0:3] = b"\x01\x02\x03"
    far[P.CHUNK - 3:] = b"\x01\x02\x03"
    out = {
        "run": b"\x41" * (2 * 258 + 5 + 1),                           # one literal, then 258 + 258 + 5 at distance 1
        "norepeat": bytes(range(256)),                                # no three bytes occur twice
        "single": b"\x07",
        "two": b"\x07\x09",                                           # fewer than three bytes: never hashed
        "distances": b"".join(_period(d, 16 * d) for d in (1, 2, 3, 4)),
        "far": bytes(far),                                            # 01 02 03 at 0 and at CHUNK - 3: the largest distance with three bytes left
        "past_end": b"\x55" * (P.CHUNK + 100),                        # a run over the chunk border: the match stops with the chunk
        "noise": rs.randint(0, 256, size=2 * P.CHUNK + 1).astype(np.uint8).tobytes(),
        "text": (b"the quick brown fox jumps over the lazy dog; " * 400)[:P.CHUNK + 1],
    }
    for n in (P.CHUNK - 1, P.CHUNK, P.CHUNK + 1):
        out[f"ramp{n}"] = (np.arange(n) // 5 % 251).astype(np.uint8).tobytes()
    return out


def fibonacci_literals() -> np.ndarray:
    """Literal tokens whose counts follow the Fibonacci numbers 1, 1, 2, 3, ... 4181 (19 values, 10945 tokens < CHUNK), shuffled with a
    fixed seed: with end-of-block the unlimited Huffman tree is deeper than 15."""
    fib = [1, 1]
    while sum(fib) + fib[-1] + fib[-2] < P.CHUNK:
        fib.append(fib[-1] + fib[-2])
    tok = np.concatenate([np.full(c, 40 + 3 * k, dtype=np.uint32) for k, c in enumerate(fib)])
    np.random.RandomState(11).shuffle(tok)
    return tok


def codelength_histogram() -> np.ndarray:
    """A literal/length histogram whose code LENGTHS occur 34, 21, 13, 8, 5, 3, 2, 1, 1 times over shuffled symbols: the code-length
    alphabet's unlimited tree is deeper than 7 (found by a search over seeds; the test asserts it)."""
    rs = np.random.RandomState(23)
    lens = rs.permutation(np.arange(3, 14))[:9]
    syms = rs.permutation(256)
    hist = np.zeros(P.HIST_WORDS, dtype=np.uint32)
    at = 0
    for nsym, length in zip([34, 21, 13, 8, 5, 3, 2, 1, 1], lens):
        for _ in range(nsym):
            hist[syms[at]] = max(1, 1 << (13 - int(length)))
            at += 1
    hist[P.EOB] = 1
    return hist


def tokens_of_histogram(hist: np.ndarray, seed: int) -> np.ndarray:
    """Literal tokens with exactly the histogram's literal counts, shuffled."""
    tok = np.concatenate([np.full(int(hist[s]), s, dtype=np.uint32) for s in range(256)])
    np.random.RandomState(seed).shuffle(tok)
    return tok


@functools.lru_cache(maxsize=None)
def token_cases():
    """name -> (tokens uint32, histogram): what the codes and emit stages are fed directly, bypassing the token stage."""
    fib = fibonacci_literals()
    cl = codelength_histogram()
    cl_tok = tokens_of_histogram(cl, 5)
    return {"fibonacci": (fib, M.histogram_of(fib)), "codelengths": (cl_tok, M.histogram_of(cl_tok))}


@functools.lru_cache(maxsize=None)
def stream_reference(name: str):
    """-> (per chunk (tokens, histogram, Block, Bits), the zlib stream)."""
    data = streams()[name]
    return M.deflate_chunks(data), M.zlib_stream(data)


def literal_bytes(tok: np.ndarray) -> bytes:
    return tok.astype(np.uint8).tobytes()
