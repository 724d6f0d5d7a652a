"""Plain numpy restatement of the quality report — used by tests only, and normative: the kernels of
ccedit_amd/csrc/quality.hip and the host code of ccedit_amd/quality.py must equal it bit for bit.  Everything is integer arithmetic;
the quotient of an SSIM window is formed with Python integers.  Floating point appears only in derive_*: PSNR, SSIM and means from the
exact integers.

The motion comes from the propagation's matcher and the mask tracker's selection (tests/_propagate_numpy.py, tests/_masktrack_numpy.py:
imported, not restated).  The constants are restated here on purpose; tests/test_quality.py checks that ccedit_amd/quality.py holds the
same.
"""
import math

import numpy as np

from _masktrack_numpy import select
from _propagate_numpy import luma, match, pyramid

WINDOW = 8
STRIDE = 4
C1 = 26634                  # (0.01 * 255)^2 * 4096, rounded
C2 = 239708                 # (0.03 * 255)^2 * 4096, rounded
Q_ONE = 1 << 32
KEEP_BELOW = 128
FB_LIMIT = 1
PAIR_CHUNK = 32


def window_terms(ya, yb):
    """Lumas uint8 (H, W) -> (Nw, Dw) as object arrays of Python integers, one entry per window at (4 i, 4 j)."""
    h, w = ya.shape
    ny, nx = (h - WINDOW) // STRIDE + 1, (w - WINDOW) // STRIDE + 1
    a, b = ya.astype(np.int64), yb.astype(np.int64)

    def wsum(img):
        s = np.zeros((ny, nx), np.int64)
        for i in range(WINDOW):
            for j in range(WINDOW):
                s += img[i:i + STRIDE * (ny - 1) + 1:STRIDE, j:j + STRIDE * (nx - 1) + 1:STRIDE]
        return s.astype(object)

    s1, s2, saa, sbb, sab = wsum(a), wsum(b), wsum(a * a), wsum(b * b), wsum(a * b)
    n = WINDOW * WINDOW
    va, vb, cov = n * saa - s1 * s1, n * sbb - s2 * s2, n * sab - s1 * s2
    return (2 * s1 * s2 + C1) * (2 * cov + C2), (s1 * s1 + s2 * s2 + C1) * (va + vb + C2)


def quotient(nw, dw):
    """q = sign(Nw) floor(|Nw| 2^32 / Dw), Python integers."""
    nw, dw = int(nw), int(dw)
    q = (abs(nw) << 32) // dw
    return -q if nw < 0 else q


def pair_frame(a, b, mask=None):
    """a, b: uint8 (H, W, 3); mask: uint8 (H, W) or None -> the eight Python integers of one frame."""
    h, w = a.shape[:2]
    kept = np.ones((h, w), bool) if mask is None else mask < KEEP_BELOW
    d = a.astype(np.int64) - b.astype(np.int64)
    sse = [int((d[..., c] ** 2)[kept].sum()) for c in range(3)]
    ya, yb = luma(a), luma(b)
    nw, dw = window_terms(ya, yb)
    ny, nx = nw.shape
    whole = np.ones((ny, nx), bool)
    for i in range(WINDOW):
        for j in range(WINDOW):
            whole &= kept[i:i + STRIDE * (ny - 1) + 1:STRIDE, j:j + STRIDE * (nx - 1) + 1:STRIDE]
    qsum = sum(quotient(nw[i, j], dw[i, j]) for i, j in zip(*np.nonzero(whole)))
    return sse + [int(kept.sum()), int(qsum), int(whole.sum()), int(ya.astype(np.int64)[kept].sum()), int(yb.astype(np.int64)[kept].sum())]


def pair(a, b, mask=None):
    """a, b: uint8 (N, H, W, 3); mask: uint8 (N, H, W) or None -> [N][8] Python integers (slot 4 signed)."""
    return [pair_frame(a[n], b[n], None if mask is None else mask[n]) for n in range(a.shape[0])]


def warp(x, y, vsel, pairs, mask=None, limit=FB_LIMIT, sel=0):
    """x: uint8 (F, H, W, 3); y: the same shape or None; vsel: int (2 P, H, W, 2); pairs: int (2 P, 4); mask: uint8 (F, H, W) or None
    -> [P][4] Python integers (SSE of x, SSE of y, valid, selected)."""
    nf, h, w = x.shape[:3]
    assert sel == 0 or mask is not None
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    out = []
    for j in range(len(pairs) // 2):
        f, g = (int(np.clip(int(pairs[2 * j][i]), 0, nf - 1)) for i in (0, 1))
        v, r = np.asarray(vsel[2 * j]).astype(np.int64), np.asarray(vsel[2 * j + 1]).astype(np.int64)
        chosen = np.ones((h, w), bool) if sel == 0 else (mask[f] >= KEEP_BELOW) if sel == 1 else (mask[f] < KEEP_BELOW)
        qy0, qx0 = ys + v[..., 0], xs + v[..., 1]
        inside = (qy0 >= 0) & (qy0 < h) & (qx0 >= 0) & (qx0 < w)
        qy, qx = np.clip(qy0, 0, h - 1), np.clip(qx0, 0, w - 1)
        rq = r[qy, qx]
        valid = chosen & inside & (np.abs(v[..., 0] + rq[..., 0]) + np.abs(v[..., 1] + rq[..., 1]) <= limit)

        def sse(seq):
            if seq is None:
                return 0
            d = seq[f].astype(np.int64) - seq[g].astype(np.int64)[qy, qx]
            return int((d ** 2).sum(axis=-1)[valid].sum())

        out.append([sse(x), sse(y), int(valid.sum()), int(chosen.sum())])
    return out


def pair_rows(frames):
    """int32 (2 (F - 1), 4): for i = 1 ... F - 1 the rows (i, i - 1, 0, 0) and (i - 1, i, 0, 0)."""
    rows = []
    for i in range(1, frames):
        rows += [(i, i - 1, 0, 0), (i - 1, i, 0, 0)]
    return np.asarray(rows, np.int32).reshape(-1, 4)


def fields(guide, rows=None):
    """guide: uint8 (F, H, W, 3) -> (rows, per-pixel vectors int32 (2 (F - 1), H, W, 2)) of the adjacent pairs: the matcher, then the
    selection."""
    rows = pair_rows(guide.shape[0]) if rows is None else rows
    pyr = [pyramid(luma(f)) for f in guide]
    return rows, np.stack([select(pyr[f][0], pyr[g][0], match(pyr[f], pyr[g])) for f, g in rows[:, :2]])


# ---- what the host derives from the integers
def _ratio(a, b):
    return None if b == 0 else a / b


def _psnr(sse, samples):
    return None if sse == 0 or samples == 0 else 10.0 * math.log10(65025 * samples / sse)


def _flicker(m):
    if len(m) < 2 or any(v is None for v in m):
        return None
    return sum(abs(b - a) for a, b in zip(m, m[1:])) / (len(m) - 1)


def derive_compare(rows):
    sse = [sum(r[c] for r in rows) for c in range(3)]
    count, qsum, windows = (sum(r[i] for r in rows) for i in (3, 4, 5))
    mean_a, mean_b = [_ratio(r[6], r[3]) for r in rows], [_ratio(r[7], r[3]) for r in rows]
    return {"frames": [dict(sse=list(r[:3]), count=r[3], q_sum=r[4], windows=r[5], luma_a=r[6], luma_b=r[7]) for r in rows],
            "sse": sse, "count": count, "q_sum": qsum, "windows": windows, "identical": count > 0 and sum(sse) == 0,
            "psnr": _psnr(sum(sse), 3 * count), "psnr_rgb": [_psnr(s, count) for s in sse],
            "ssim": None if windows == 0 else qsum / (windows * Q_ONE), "mean_luma_a": mean_a, "mean_luma_b": mean_b,
            "flicker": {"a": _flicker(mean_a), "b": _flicker(mean_b)}}


def warp_mse(rows, slot=0):
    valid = sum(r[2] for r in rows)
    return _ratio(sum(r[slot] for r in rows), 3 * valid)


def valid_share(rows):
    return _ratio(sum(r[2] for r in rows), sum(r[3] for r in rows))


def report(source, result, mask=None):
    """The dict of ccedit_amd.quality.report from the restatement's integers.  mask: uint8 (F, H, W) or None."""
    n, h, w = source.shape[:3]
    fid = derive_compare(pair(source, result, mask))
    out = {"size": [h, w], "frames": n, "masked": mask is not None,
           "fidelity": {k: v for k, v in fid.items() if k != "flicker"},
           "flicker": {"source": fid["flicker"]["a"], "result": fid["flicker"]["b"]}, "temporal": None}
    if n < 2 or h % 64 or w % 64:
        return out
    rows, vsel = fields(source)
    out["temporal"] = {}
    for name, sel in (("all", 0),) + ((("edited", 1),) if mask is not None else ()):
        t = warp(result, source, vsel, rows, mask, FB_LIMIT, sel)
        r, s = warp_mse(t, 0), warp_mse(t, 1)
        out["temporal"][name] = {"result": r, "source": s, "ratio": None if r is None or not s else r / s, "valid_share": valid_share(t),
                                 "pairs": [[int(a), int(b)] for a, b in rows[0::2, :2]], "sse_result": [v[0] for v in t],
                                 "sse_source": [v[1] for v in t], "valid": [v[2] for v in t], "selected": [v[3] for v in t]}
    return out
