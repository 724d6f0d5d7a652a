"""Plain numpy restatement of mask tracking — used by tests only, and normative: the kernels of
ccedit_amd/csrc/masktrack.hip and ccedit_mask_dilate must equal it bit for bit.  Everything is integer arithmetic.

A mask painted on frame K is carried to every frame of the clip, one frame at a time moving away from K.  For frame f with its
neighbour g on K's side: block vectors f -> g and g -> f from the propagation's matcher (tests/_propagate_numpy.py, imported, not
restated) -> per pixel the best of the 3 x 3 neighbouring blocks' vectors by a 5 x 5 box sum of absolute luma differences -> a
nearest lookup of g's mask, cleared where the two directions disagree by more than FB_LIMIT (a pixel that frame g does not show).
The constants are restated here on purpose; tests/test_masktrack.py checks that ccedit_amd/masktrack.py holds the same.
"""
import numpy as np

from _propagate_numpy import BLOCK, luma, match, pyramid  # noqa: F401  (luma and pyramid are re-exported for the tests)

# (dby, dbx) of the candidate blocks, in the order that breaks ties: the minimum of S * 16 + order wins
CANDIDATES = ((0, 0), (-1, 0), (0, -1), (0, 1), (1, 0), (-1, -1), (-1, 1), (1, -1), (1, 1))
BOX = 5                     # side of the box sum
FB_LIMIT = 1                # largest |v(p) + r(q)|_1 of a consistent correspondence
VEC_MAX = 64                # block vectors are clamped into +-VEC_MAX before use (the matcher's own reach is 46)
DILATE_MAX = 32


def select(yf, yg, vec):
    """yf, yg: uint8 (H, W); vec: int (H / 8, W / 8, 2) block vectors (dy, dx) from yf into yg -> int32 (H, W, 2): per pixel the
    candidate c among the 3 x 3 neighbouring blocks' vectors (indices clamped) of minimum S_c * 16 + order, S_c the 5 x 5 box sum
    (edge-replicated) of d_c(p) = |yf(p) - yg(clamp(p + c))| with ONE c — that of the pixel's own block — over the whole box."""
    h, w = yf.shape
    nby, nbx = h // BLOCK, w // BLOCK
    vec = np.clip(np.asarray(vec).astype(np.int64), -VEC_MAX, VEC_MAX)
    a, b = yf.astype(np.int32), yg.astype(np.int32)
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    r = BOX // 2
    best_key = np.full((h, w), np.iinfo(np.int64).max, np.int64)
    best = np.zeros((h, w, 2), np.int64)
    for order, (dby, dbx) in enumerate(CANDIDATES):
        c = vec[np.clip((ys >> 3) + dby, 0, nby - 1), np.clip((xs >> 3) + dbx, 0, nbx - 1)]            # (h, w, 2)
        s = np.zeros((h, w), np.int64)
        for i in range(-r, r + 1):
            for j in range(-r, r + 1):
                py, px = np.clip(ys + i, 0, h - 1), np.clip(xs + j, 0, w - 1)                           # edge replication of d_c
                s += np.abs(a[py, px] - b[np.clip(py + c[..., 0], 0, h - 1), np.clip(px + c[..., 1], 0, w - 1)])
        key = s * 16 + order
        better = key < best_key
        best_key = np.where(better, key, best_key)
        best[better] = c[better]
    return best.astype(np.int32)


def step(m_g, v, r, limit=FB_LIMIT):
    """m_g: uint8 (H, W); v: (H, W, 2) per-pixel vectors f -> g; r: those g -> f.  -> m_f: m_g at q = clamp(p + v(p)), or 0 where
    |v_y(p) + r_y(q)| + |v_x(p) + r_x(q)| > limit."""
    h, w = m_g.shape
    v, r = v.astype(np.int64), r.astype(np.int64)
    qy = np.clip(np.arange(h)[:, None] + v[..., 0], 0, h - 1)
    qx = np.clip(np.arange(w)[None, :] + v[..., 1], 0, w - 1)
    rq = r[qy, qx]
    bad = np.abs(v[..., 0] + rq[..., 0]) + np.abs(v[..., 1] + rq[..., 1]) > limit
    return np.where(bad, 0, m_g[qy, qx]).astype(np.uint8)


def track(frames, anchor_mask, anchor, limit=FB_LIMIT):
    """frames: uint8 (F, H, W, 3); anchor_mask: uint8 (H, W) painted on frame `anchor` -> uint8 (F, H, W): the mask of every frame."""
    n = frames.shape[0]
    pyr = [pyramid(luma(f)) for f in frames]
    out = np.zeros(frames.shape[:3], np.uint8)
    out[anchor] = anchor_mask
    for f, g in [(f, f - 1) for f in range(anchor + 1, n)] + [(f, f + 1) for f in range(anchor - 1, -1, -1)]:
        v = select(pyr[f][0], pyr[g][0], match(pyr[f], pyr[g]))
        r = select(pyr[g][0], pyr[f][0], match(pyr[g], pyr[f]))
        out[f] = step(out[g], v, r, limit)
    return out


def dilate(m, radius):
    """uint8 (..., H, W) -> the (2 radius + 1)^2 square maximum, the window clipped at the border."""
    if radius == 0:
        return m.copy()
    h, w = m.shape[-2:]
    p = np.pad(m, [(0, 0)] * (m.ndim - 2) + [(radius, radius), (radius, radius)], mode="constant")        # bytes are >= 0: padding never wins
    rows = np.max(np.stack([p[..., radius:radius + h, j:j + w] for j in range(2 * radius + 1)]), axis=0)
    p = np.pad(rows, [(0, 0)] * (m.ndim - 2) + [(radius, radius), (0, 0)], mode="constant")
    return np.max(np.stack([p[..., i:i + h, :] for i in range(2 * radius + 1)]), axis=0).astype(np.uint8)


def invert(m):
    return (255 - m).astype(np.uint8)


def finish(m, radius=0, inverted=False):
    """What follows tracking, in this order: dilate, then invert."""
    m = dilate(m, radius)
    return invert(m) if inverted else m


def iou(a, b):
    a, b = a >= 128, b >= 128
    u = np.logical_or(a, b).sum()
    return 1.0 if u == 0 else float(np.logical_and(a, b).sum()) / float(u)
