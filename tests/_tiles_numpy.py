"""Large frames (ccedit_amd/tiles.py, csrc/tile.hip) restated in numpy float32, with the operation order of the definition: the plan,
the gather and the fuse.  Written from the definition alone (no import from ccedit_amd), so that the tests compare two statements."""
import numpy as np


def axis_starts(n, t, o):
    """k * (t - o) while that tile ends before the frame does, then n - t."""
    out, k = [], 0
    while k * (t - o) + t < n:
        out.append(k * (t - o))
        k += 1
    return out + [n - t]


def raw_weight(t):
    return np.array([min(k + 1, t - k) for k in range(t)], np.int64)


def tables(h, w, th, tw, starts):
    """coef float32 (tiles, th, tw) for ANY list of (sy, sx) starts: raw / D from integers in float64, rounded to fp32 once."""
    raw = raw_weight(th)[:, None] * raw_weight(tw)[None, :]
    total = np.zeros((h, w), np.int64)
    for sy, sx in starts:
        total[sy:sy + th, sx:sx + tw] += raw
    coef = np.empty((len(starts), th, tw), np.float32)
    for t, (sy, sx) in enumerate(starts):
        coef[t] = (raw.astype(np.float64) / total[sy:sy + th, sx:sx + tw].astype(np.float64)).astype(np.float32)
    return coef


def plan2d(lh, lw, th, tw, oh, ow):
    starts = [(sy, sx) for sy in axis_starts(lh, th, oh) for sx in axis_starts(lw, tw, ow)]
    return starts, tables(lh, lw, th, tw, starts)


def clamp_starts(starts, h, w, th, tw):
    """What the kernels make of a table: every start held inside 0 ... h - th / 0 ... w - tw."""
    return [(min(max(int(sy), 0), h - th), min(max(int(sx), 0), w - tw)) for sy, sx in starts]


def gather(x, starts, th, tw):
    """x (..., h, w) -> (tiles, ..., th, tw): copies."""
    return np.stack([x[..., sy:sy + th, sx:sx + tw] for sy, sx in starts]).astype(np.float32)


def fuse(ys, starts, coef, h, w):
    """ys: tiles of (..., th, tw) float32 -> (..., h, w).  Per element the tiles in ascending order; the first term is the product
    alone, every further term one multiply (rounded) then one add (rounded); an element no tile covers is 0."""
    th, tw = ys[0].shape[-2:]
    out = np.zeros(ys[0].shape[:-2] + (h, w), np.float32)
    seen = np.zeros((h, w), bool)
    for t, (sy, sx) in enumerate(starts):
        term = (coef[t].astype(np.float32) * ys[t].astype(np.float32)).astype(np.float32)
        region = out[..., sy:sy + th, sx:sx + tw]
        first = ~seen[sy:sy + th, sx:sx + tw]
        out[..., sy:sy + th, sx:sx + tw] = np.where(first, term, (region + term).astype(np.float32))
        seen[sy:sy + th, sx:sx + tw] = True
    return out
