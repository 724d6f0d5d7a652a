"""Plain numpy restatement of motion-following noise — used by tests only, and normative: the kernels of
ccedit_amd/csrc/noisewarp.hip and ccedit_amd/noisewarp.py's build must equal it bit for bit.  Everything is integer arithmetic and
bit copies.

Once per clip it is decided which noise sample every latent cell (8 x 8 pixels) of every keyframe inherits from an earlier keyframe,
along the source's motion: block vectors between adjacent source frames in both directions from the propagation's matcher
(tests/_propagate_numpy.py, imported, not restated) -> the centre of every cell followed frame by frame back to the previous keyframe,
dropped where it leaves the frame or the two directions disagree by more than FB_LIMIT (track) -> the position the cell's sample had
when it was first drawn, found through the previous keyframe's origins; where several cells of a keyframe arrive at one sample the
smallest cell index keeps it, the others draw fresh (origins) -> an index map into the clip's flattened (K, cells) noise (src), a
permutation-free gather: every frame reads distinct samples, so the noise of every single frame stays white.
The constants are restated here on purpose; tests/test_noisewarp.py checks that ccedit_amd/noisewarp.py holds the same.
"""
import numpy as np

from _propagate_numpy import BLOCK, luma, match, pyramid  # noqa: F401

CELL = 8                    # a latent cell is 8 x 8 pixels = one block of the matcher
FB_LIMIT = 4                # largest |v(p) + r(q)|_1 of a consistent correspondence
VEC_MAX = 64                # block vectors are clamped into +-VEC_MAX where they are read
TABLE_MAX = 2 ** 32 - 1     # K * cells must stay below it: a claim is k * cells + (cells - 1 - idx) + 1 in 32 bits


def pair_rows(frames):
    """For frame f = 1 ... frames - 1: row (f, f - 1) and then row (f - 1, f) -> [(f, g)] of 2 (frames - 1) rows."""
    rows = []
    for f in range(1, frames):
        rows += [(f, f - 1), (f - 1, f)]
    return rows


def vectors(frames):
    """uint8 (F, H, W, 3) -> int32 (2 (F - 1), H / 8, W / 8, 2): the matcher's block vectors (dy, dx) of pair_rows."""
    pyr = [pyramid(luma(f)) for f in frames]
    h, w = frames.shape[1] // CELL, frames.shape[2] // CELL
    out = [match(pyr[f], pyr[g]) for f, g in pair_rows(frames.shape[0])]
    return np.asarray(out, np.int32).reshape(-1, h, w, 2)


def centres(h, w):
    """-> (cy, cx), int64 (h w,): the centre pixel (8 i + 4, 8 j + 4) of every cell in linear order."""
    i, j = np.divmod(np.arange(h * w, dtype=np.int64), w)
    return CELL * i + CELL // 2, CELL * j + CELL // 2


def track(vec, key, H, W, limit=FB_LIMIT):
    """vec: int (2 (F - 1), h, w, 2) in pair_rows' order; key: the keyframes' frame numbers, key[0] = 0, strictly increasing
    -> int32 (K, cells, 3) = (valid, Q_y, Q_x); row 0 is zero.  From the cell's centre in frame key[k], for f = key[k] down to
    key[k - 1] + 1: v = vec(f -> f - 1) at cell p >> 3, q = p + v, inside = q in the frame (before clamping), q clamped,
    r = vec(f - 1 -> f) at cell q >> 3, valid &= inside & (|v_y + r_y| + |v_x + r_x| <= limit), p = q."""
    h, w = H // CELL, W // CELL
    vec = np.clip(np.asarray(vec).astype(np.int64), -VEC_MAX, VEC_MAX)
    out = np.zeros((len(key), h * w, 3), np.int32)
    for k in range(1, len(key)):
        py, px = centres(h, w)
        valid = np.ones(h * w, bool)
        for f in range(int(key[k]), int(key[k - 1]), -1):
            v = vec[2 * (f - 1)][py >> 3, px >> 3]
            qy, qx = py + v[:, 0], px + v[:, 1]
            inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
            qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
            r = vec[2 * (f - 1) + 1][qy >> 3, qx >> 3]
            valid &= inside & (np.abs(v[:, 0] + r[:, 0]) + np.abs(v[:, 1] + r[:, 1]) <= limit)
            py, px = qy, qx
        out[k] = np.stack([valid.astype(np.int64), py, px], axis=1)
    return out


def origins(trk, H, W):
    """trk: int (K, cells, 3) from track -> (org int32 (K, cells, 3) = (R, P_y, P_x), src int32 (K, cells), inherited int64 (K,)).
    org[0] = (0, centre).  For k >= 1 and a valid cell: c' = Q >> 3, d = Q - centre(c'), (R', P') = org[k - 1][c'], P = P' + d; a
    candidate iff P is in the frame, with the key R' cells + (P_y >> 3) w + (P_x >> 3); of the candidates that share a key the smallest
    linear cell index gets (R', P), every other cell is fresh: (k, own centre).  src = R cells + (P_y >> 3) w + (P_x >> 3);
    inherited[k] counts the cells of keyframe k with R != k."""
    h, w = H // CELL, W // CELL
    cells = h * w
    K = trk.shape[0]
    cy, cx = centres(h, w)
    trk = np.asarray(trk).astype(np.int64)
    org = np.zeros((K, cells, 3), np.int64)
    org[0] = np.stack([np.zeros(cells, np.int64), cy, cx], axis=1)
    for k in range(1, K):
        valid, qy, qx = trk[k, :, 0] != 0, np.clip(trk[k, :, 1], 0, H - 1), np.clip(trk[k, :, 2], 0, W - 1)
        cq = (qy >> 3) * w + (qx >> 3)
        prev = org[k - 1][cq]
        ry = prev[:, 1] + (qy & 7) - CELL // 2
        rx = prev[:, 2] + (qx & 7) - CELL // 2
        cand = valid & (ry >= 0) & (ry < H) & (rx >= 0) & (rx < W)
        keys = prev[:, 0] * cells + (np.clip(ry, 0, H - 1) >> 3) * w + (np.clip(rx, 0, W - 1) >> 3)
        idx = np.nonzero(cand)[0]                                   # ascending: the first occurrence of a key is its smallest index
        _, first = np.unique(keys[idx], return_index=True)
        win = np.zeros(cells, bool)
        win[idx[first]] = True
        org[k] = np.stack([np.full(cells, k, np.int64), cy, cx], axis=1)
        org[k][win] = np.stack([prev[win, 0], ry[win], rx[win]], axis=1)
    src = org[..., 0] * cells + (org[..., 1] >> 3) * w + (org[..., 2] >> 3)
    inherited = (org[..., 0] != np.arange(K)[:, None]).sum(axis=1)
    return org.astype(np.int32), src.astype(np.int32), inherited.astype(np.int64)


def build(frames, key_index):
    """frames: uint8 (F, H, W, 3), all source frames; key_index: the keyframes' frame numbers, strictly increasing
    -> (src int32 (K, cells), shares float64 (K,) = inherited / cells).  Only the frames key[0] ... key[K - 1] take part."""
    key = np.asarray([int(i) for i in key_index], np.int64)
    H, W = frames.shape[1:3]
    if key.size * (H // CELL) * (W // CELL) >= TABLE_MAX:
        raise ValueError("too many cells")
    part = frames[key[0]:key[-1] + 1]
    vec = vectors(part) if part.shape[0] > 1 else np.zeros((0, H // CELL, W // CELL, 2), np.int32)
    _, src, inherited = origins(track(vec, key - key[0], H, W), H, W)
    return src, inherited / float((H // CELL) * (W // CELL))


def gather(raw, src):
    """raw: (B, C, K, h, w) of any 4-byte type; src: int (B, K, cells) -> out[b][c][k][cell] = raw[b][c].flat[src[b][k][cell]]: a bit copy."""
    b, c, k, h, w = raw.shape
    bits = np.ascontiguousarray(raw).view(np.uint32).reshape(b, c, k * h * w)
    out = np.stack([bits[i][:, np.asarray(src[i]).reshape(-1).astype(np.int64)] for i in range(b)])
    return out.reshape(b, c, k, h, w).view(raw.dtype)
