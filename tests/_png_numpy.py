"""The PNG / deflate format of ccedit_amd/png.py restated in numpy and plain Python: the DEFINITION the kernels of csrc/png.hip equal byte
for byte.  Constants come from ccedit_amd/png.py (their one place).  Integer arithmetic only.

filter_frame    Per row the filter t in (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth) with the smallest sum over the row's 3 W bytes of
                min(v, 256 - v), ties to the lowest t.  a = the byte 3 to the left, b = the byte above, c = above-left; outside the image 0
                (also the whole row above row 0).  Filters read SOURCE bytes.  -> H * (1 + 3 W) bytes.
tokens          A chunk b[0 .. n-1] is walked greedily from i = 0:
                  * if i + 3 <= n: h = ((b[i] | b[i+1] << 8 | b[i+2] << 16) * HASH_MUL mod 2^32) >> (32 - HASH_BITS); cand = table[h];
                    table[h] = i (ALWAYS, before the comparison).  If cand is not empty, L = the number of equal bytes b[cand + k] ==
                    b[i + k], k < min(MAX_MATCH, n - i): a match never runs past the chunk's end, and may overlap itself (distance <
                    length).  L >= 3: a match token (L, i - cand), every position j = i + 1 ... i + L - 1 that still has three bytes
                    (j + 3 <= n) is entered into the table (table[hash at j] = j, in rising j: worth 7 % of the file on the real
                    frame of tests/golden), i += L.
                  * otherwise (no candidate, L < 3, or fewer than 3 bytes left: the chunk's last two bytes are always literals):
                    literal b[i], i += 1.
                The table starts empty with every chunk; it has HASH_SIZE entries and no chains.  Histograms: 286 literal/length symbols
                (end-of-block counted once) at 0, 30 distance symbols at DIST_AT.
code_lengths    counts -> lengths limited to max_bits.  The used symbols are sorted by (count, symbol) ascending.  None used: all 0.  One:
                length 1.  Otherwise the two-queue Huffman construction: leaves in sorted order, internal nodes in creation order; the
                next node is the head of the leaf queue if it exists and weighs LESS than the head of the internal queue (or that is empty),
                else the head of the internal queue: on equal weights the older subtree goes first.  Leaf depths (the maximum is `unlimited`) are clamped to max_bits into count-per-length
                n[.]; REPAIR while sum n[l] 2^(max_bits - l) > 2^max_bits: n[max_bits] -= 1; for the largest l < max_bits with n[l] > 0:
                n[l] -= 1, n[l + 1] += 2 — a leaf of level l becomes an inner node over itself and the leaf taken from the deepest
                level, which lowers the Kraft sum by exactly one unit of 2^-max_bits and keeps the number of leaves.  The lengths are
                handed out from max_bits down to 1 along the sorted order: rarer symbols, and among equals lower numbers, get the longer ones.
                With two or more used symbols the code is complete (Kraft sum exactly 1).
canonical codes code(s) per length in symbol order from next[l] = (next[l - 1] + n[l - 1]) << 1; sent most significant bit first.
header          BFINAL, BTYPE = 2, HLIT = (last used literal/length symbol + 1) - 257, HDIST = max(last used distance symbol + 1, 1) - 1;
                the HLIT + 257 + HDIST + 1 lengths as ONE sequence, run-coded greedily from i = 0 over run = the number of equal entries
                from i on: value 0 and run >= 3: r = min(run, 138), code 17 (r <= 10, 3 extra bits r - 3) or 18 (7 extra bits r - 11),
                i += r; value v > 0 and run >= 4: v, then 16 with r = min(run - 1, 6) (2 extra bits r - 3), i += 1 + r; else v, i += 1.
                The 19 code-length symbols get lengths limited to 7 by code_lengths; HCLEN trims CL_ORDER's unused tail (at least 4 sent).
                Literal/length always has two used symbols (a literal or a length, and end-of-block), and at least 257 lengths are
                sent, which cannot all be one non-zero value (257 is no power of two): the sequence holds two different code-length
                symbols at least, so the code-length code is complete too.
chunk bits      header, then per token the literal's code, or length code + extra bits + distance code + extra bits; end-of-block.
stream          78 01, the chunks' bits back to back (LSB first), zero padding to a byte, Adler-32 of the filtered bytes, big-endian.

HEADER_MAX (png.py), the condition on noise.  A chunk WITHOUT a match holds n literals and one end-of-block: at most 257 symbols.  A
Huffman code is no longer than any other prefix code for the same counts, so no longer than "255 literal values at 8 bits, the rarest
literal value and end-of-block at 9": 8 n + (count of the rarest value <= n / 256) + 9 bits.  (The repair acts only when the unlimited
tree is deeper than 15, which takes counts that grow like the Fibonacci numbers: the rarest of 16 such symbols would have to be rarer
than 1 in 1597, and noise has no such symbol in a chunk of 16384 bytes.)  The header is at most HEADER_MAX_BITS.  Hence HEADER_MAX =
ceil((HEADER_MAX_BITS + CHUNK / 256 + 9) / 8) bytes per chunk beyond the raw bytes.  Noise does hold the odd three-byte repeat (about
CHUNK^2 / 2^25 = 8 hash hits a chunk that compare equal by chance): such a match costs at most 48 bits for 3 bytes, 24 more than
literals, and the real header (about 150 of the 563 bytes allowed) leaves room for a hundred of them; the test asserts the bound on the file.
"""
from __future__ import annotations

import struct
import zlib

import numpy as np

from ccedit_amd import png as P

_LEN_BASE = np.array(P.LEN_BASE)
_DIST_BASE = np.array(P.DIST_BASE)


# ------------------------------------------------------------------------------------------ filtering
def filter_frame(frame: np.ndarray) -> np.ndarray:
    """uint8 (H, W, 3) -> uint8 (H, 1 + 3 W)."""
    h, w, _ = frame.shape
    x = frame.reshape(h, 3 * w).astype(np.int32)
    a = np.zeros_like(x)
    a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, 3:] = x[:-1, :-3]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cand = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth], axis=0) & 255          # (5, H, 3W)
    cost = np.minimum(cand, 256 - cand).sum(axis=2)                                          # (5, H)
    pick = np.argmin(cost, axis=0)                                                           # the first minimum: the lowest filter number
    out = np.empty((h, 1 + 3 * w), dtype=np.uint8)
    out[:, 0] = pick
    out[:, 1:] = cand[pick, np.arange(h)]
    return out


def unfilter(filtered: np.ndarray, h: int, w: int) -> np.ndarray:
    """The PNG decoder's reconstruction, independent of filter_frame: bytes (H * (1 + 3 W),) -> uint8 (H, W, 3)."""
    rows = np.frombuffer(bytes(filtered), dtype=np.uint8).reshape(h, 1 + 3 * w)
    out = np.zeros((h, 3 * w), dtype=np.int32)
    for y in range(h):
        t = int(rows[y, 0])
        up = out[y - 1] if y else np.zeros(3 * w, dtype=np.int32)
        cur = out[y]
        src = rows[y, 1:].astype(np.int32)
        if t == 0:
            cur[:] = src
        elif t == 2:
            cur[:] = (src + up) & 255
        else:
            for i in range(3 * w):
                a = cur[i - 3] if i >= 3 else 0
                b = up[i]
                c = up[i - 3] if i >= 3 else 0
                if t == 1:
                    pred = a
                elif t == 3:
                    pred = (a + b) >> 1
                else:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cur[i] = (src[i] + pred) & 255
    return out.astype(np.uint8).reshape(h, w, 3)


# ------------------------------------------------------------------------------------------ LZ77
def length_symbol(length: int):
    """-> (symbol, extra bits, extra value)."""
    if length == P.MAX_MATCH:
        return 285, 0, 0
    k = int(np.searchsorted(_LEN_BASE, length, side="right")) - 1
    return 257 + k, P.LEN_EXTRA[k], length - P.LEN_BASE[k]


def dist_symbol(dist: int):
    k = int(np.searchsorted(_DIST_BASE, dist, side="right")) - 1
    return k, P.DIST_EXTRA[k], dist - P.DIST_BASE[k]


def tokens(chunk: bytes):
    """One chunk's bytes -> (token words uint32 (ntok,), histogram uint32 (HIST_WORDS,))."""
    b = bytes(chunk)
    n = len(b)
    assert 1 <= n
    table = {}
    out = []
    hist = np.zeros(P.HIST_WORDS, dtype=np.uint32)
    shift = 32 - P.HASH_BITS
    i = 0
    while i < n:
        length = 0
        if i + 3 <= n:
            h = (((b[i] | b[i + 1] << 8 | b[i + 2] << 16) * P.HASH_MUL) & 0xffffffff) >> shift
            cand = table.get(h)
            table[h] = i
            if cand is not None:
                top = min(P.MAX_MATCH, n - i)
                while length < top and b[cand + length] == b[i + length]:
                    length += 1
        if length >= P.MIN_MATCH:
            out.append(P.TOKEN_MATCH | (length - 3) << 16 | (i - cand - 1))
            hist[length_symbol(length)[0]] += 1
            hist[P.DIST_AT + dist_symbol(i - cand)[0]] += 1
            for j in range(i + 1, min(i + length, n - 2)):
                table[(((b[j] | b[j + 1] << 8 | b[j + 2] << 16) * P.HASH_MUL) & 0xffffffff) >> shift] = j
            i += length
        else:
            out.append(b[i])
            hist[b[i]] += 1
            i += 1
    hist[P.EOB] += 1
    return np.array(out, dtype=np.uint32), hist


def histogram_of(tok: np.ndarray) -> np.ndarray:
    hist = np.zeros(P.HIST_WORDS, dtype=np.uint32)
    for t in tok.tolist():
        if t & P.TOKEN_MATCH:
            hist[length_symbol(((t >> 16) & 255) + 3)[0]] += 1
            hist[P.DIST_AT + dist_symbol((t & 0xffff) + 1)[0]] += 1
        else:
            hist[t] += 1
    hist[P.EOB] += 1
    return hist


# ------------------------------------------------------------------------------------------ Huffman
def code_lengths(counts, max_bits: int):
    """counts (n,) -> (lengths (n,) int, unlimited depth of the Huffman tree)."""
    counts = [int(c) for c in counts]
    order = sorted((s for s in range(len(counts)) if counts[s] > 0), key=lambda s: (counts[s], s))
    lengths = [0] * len(counts)
    n = len(order)
    if n == 0:
        return lengths, 0
    if n == 1:
        lengths[order[0]] = 1
        return lengths, 1
    w = [counts[s] for s in order]
    iw = []
    leaf_parent = [0] * n
    int_parent = [0] * (n - 1)
    li = ii = 0
    for k in range(n - 1):
        total = 0
        for _ in range(2):
            if li < n and (ii >= len(iw) or w[li] < iw[ii]):
                leaf_parent[li] = k
                total += w[li]
                li += 1
            else:
                int_parent[ii] = k
                total += iw[ii]
                ii += 1
        iw.append(total)
    depth = [0] * (n - 1)
    for j in range(n - 3, -1, -1):
        depth[j] = depth[int_parent[j]] + 1
    per = [0] * (max_bits + 1)
    unlimited = 0
    for i in range(n):
        d = depth[leaf_parent[i]] + 1
        unlimited = max(unlimited, d)
        per[min(d, max_bits)] += 1
    total = sum(per[l] << (max_bits - l) for l in range(1, max_bits + 1))
    while total > 1 << max_bits:
        per[max_bits] -= 1
        for l in range(max_bits - 1, 0, -1):
            if per[l]:
                per[l] -= 1
                per[l + 1] += 2
                break
        total -= 1
    at = 0
    for l in range(max_bits, 0, -1):
        for _ in range(per[l]):
            lengths[order[at]] = l
            at += 1
    return lengths, unlimited


def kraft(lengths, max_bits: int) -> int:
    """The Kraft sum in units of 2^-max_bits: a complete code gives 1 << max_bits."""
    return sum(1 << (max_bits - l) for l in lengths if l)


def canonical(lengths, max_bits: int):
    """-> codes (n,), as numbers whose bit (length - 1) is sent first."""
    per = [0] * (max_bits + 2)
    for l in lengths:
        per[l] += 1
    per[0] = 0
    nxt = [0] * (max_bits + 2)
    for l in range(1, max_bits + 1):
        nxt[l] = (nxt[l - 1] + per[l - 1]) << 1
    codes = [0] * len(lengths)
    for s, l in enumerate(lengths):
        if l:
            codes[s] = nxt[l]
            nxt[l] += 1
    return codes


class Bits:
    """LSB-first bit string as a Python integer."""

    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value: int, width: int):
        self.v |= (value & ((1 << width) - 1)) << self.n
        self.n += width

    def put_code(self, code: int, length: int):
        """A Huffman code: most significant bit first."""
        self.put(int(format(code, f"0{length}b")[::-1], 2) if length else 0, length)

    def append(self, other: "Bits"):
        self.v |= other.v << self.n
        self.n += other.n

    def tobytes(self) -> bytes:
        return self.v.to_bytes((self.n + 7) // 8, "little")


def run_code(seq):
    """The code-length sequence -> [(symbol, extra bits, extra value)]."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v = seq[i]
        run = 1
        while i + run < n and seq[i + run] == v:
            run += 1
        if v == 0 and run >= 3:
            r = min(run, 138)
            out.append((17, 3, r - 3) if r <= 10 else (18, 7, r - 11))
            i += r
        elif v != 0 and run >= 4:
            r = min(run - 1, 6)
            out.append((v, 0, 0))
            out.append((16, 2, r - 3))
            i += 1 + r
        else:
            out.append((v, 0, 0))
            i += 1
    return out


class Block:
    """Everything the codes stage derives from one chunk's histograms."""

    def __init__(self, hist, final: bool):
        hist = [int(v) for v in hist]
        self.lit_len, self.lit_unlimited = code_lengths(hist[:P.LITLEN_SYMS], P.MAX_BITS)
        self.dist_len, self.dist_unlimited = code_lengths(hist[P.DIST_AT:P.DIST_AT + P.DIST_SYMS], P.MAX_BITS)
        self.lit_code = canonical(self.lit_len, P.MAX_BITS)
        self.dist_code = canonical(self.dist_len, P.MAX_BITS)
        hlit = max(s for s in range(P.LITLEN_SYMS) if self.lit_len[s]) + 1
        hdist = max([s for s in range(P.DIST_SYMS) if self.dist_len[s]] + [0]) + 1
        self.hlit, self.hdist = hlit, hdist
        self.runs = run_code(self.lit_len[:hlit] + self.dist_len[:hdist])
        cl_hist = [0] * P.CL_SYMS
        for s, _, _ in self.runs:
            cl_hist[s] += 1
        self.cl_hist = cl_hist
        self.cl_len, self.cl_unlimited = code_lengths(cl_hist, P.CL_MAX_BITS)
        self.cl_code = canonical(self.cl_len, P.CL_MAX_BITS)
        hclen = max(k for k in range(P.CL_SYMS) if self.cl_len[P.CL_ORDER[k]]) + 1
        self.hclen = max(hclen, 4)
        h = Bits()
        h.put(1 if final else 0, 1)
        h.put(2, 2)
        h.put(hlit - 257, 5)
        h.put(hdist - 1, 5)
        h.put(self.hclen - 4, 4)
        for k in range(self.hclen):
            h.put(self.cl_len[P.CL_ORDER[k]], 3)
        for s, eb, ev in self.runs:
            h.put_code(self.cl_code[s], self.cl_len[s])
            h.put(ev, eb)
        self.header = h
        body = 0
        for s in range(P.LITLEN_SYMS):
            body += hist[s] * (self.lit_len[s] + (P.LEN_EXTRA[s - 257] if s >= 257 else 0))
        for s in range(P.DIST_SYMS):
            body += hist[P.DIST_AT + s] * (self.dist_len[s] + P.DIST_EXTRA[s])
        self.bits = h.n + body

    def code_table(self) -> np.ndarray:
        """What the codes stage stores: per symbol length << 16 | the code with its bits reversed (sent LSB first)."""
        out = np.zeros(P.HIST_WORDS, dtype=np.uint32)
        for base, lens, codes in ((0, self.lit_len, self.lit_code), (P.DIST_AT, self.dist_len, self.dist_code)):
            for s, l in enumerate(lens):
                if l:
                    out[base + s] = l << 16 | int(format(codes[s], f"0{l}b")[::-1], 2)
        return out

    def header_words(self) -> np.ndarray:
        raw = self.header.v.to_bytes(P.HEADER_WORDS * 4, "little")
        return np.frombuffer(raw, dtype="<u4").copy()

    def emit(self, tok: np.ndarray) -> Bits:
        out = Bits()
        out.append(self.header)
        for t in tok.tolist():
            if t & P.TOKEN_MATCH:
                s, eb, ev = length_symbol(((t >> 16) & 255) + 3)
                out.put_code(self.lit_code[s], self.lit_len[s])
                out.put(ev, eb)
                s, eb, ev = dist_symbol((t & 0xffff) + 1)
                out.put_code(self.dist_code[s], self.dist_len[s])
                out.put(ev, eb)
            else:
                out.put_code(self.lit_code[t], self.lit_len[t])
        out.put_code(self.lit_code[P.EOB], self.lit_len[P.EOB])
        assert out.n == self.bits
        return out


# ------------------------------------------------------------------------------------------ streams and files
def adler_partial(chunk: bytes):
    """(sum of d[k], sum of (n - k) d[k]) mod 65521 of one chunk."""
    d = np.frombuffer(bytes(chunk), dtype=np.uint8).astype(np.int64)
    n = d.size
    return int(d.sum() % P.ADLER_MOD), int((d * (n - np.arange(n))).sum() % P.ADLER_MOD)


def adler_combine(parts, lens) -> int:
    s1, s2 = 1, 0
    for (a, b), n in zip(parts, lens):
        s2 = (s2 + n * s1 + b) % P.ADLER_MOD
        s1 = (s1 + a) % P.ADLER_MOD
    return s2 << 16 | s1


def split(stream: bytes, chunk: int = P.CHUNK):
    stream = bytes(stream)
    return [stream[at:at + chunk] for at in range(0, len(stream), chunk)]


def deflate_chunks(stream: bytes, chunk: int = P.CHUNK):
    """-> (per chunk (tokens, histogram, Block, Bits))."""
    parts = split(stream, chunk)
    out = []
    for k, part in enumerate(parts):
        tok, hist = tokens(part)
        blk = Block(hist, k == len(parts) - 1)
        out.append((tok, hist, blk, blk.emit(tok)))
    return out


def zlib_stream(stream: bytes, chunk: int = P.CHUNK) -> bytes:
    """Filtered (or any) bytes -> 78 01 + deflate + Adler-32.  `chunk` other than CHUNK: only for the size table in ccedit_amd/png.py."""
    stream = bytes(stream)
    bits = Bits()
    for _, _, _, b in deflate_chunks(stream, chunk):
        bits.append(b)
    parts = split(stream, chunk)
    adler = adler_combine([adler_partial(p) for p in parts], [len(p) for p in parts])
    assert adler == zlib.adler32(stream)
    return b"\x78\x01" + bits.tobytes() + struct.pack(">I", adler)


def encode_frames(frames: np.ndarray):
    """uint8 (N, H, W, 3) -> per frame its zlib stream."""
    return [zlib_stream(filter_frame(f).tobytes()) for f in frames]


def write_apng(path: str, frames: np.ndarray, duration_ms: int) -> str:
    return P.write_apng(path, encode_frames(frames), duration_ms, frames.shape[2], frames.shape[1])
