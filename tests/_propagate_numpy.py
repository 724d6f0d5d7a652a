"""Plain numpy restatement of the keyframe propagation — used by tests only, and normative: the kernels of
ccedit_amd/csrc/propagate.hip must equal it bit for bit.  Everything is integer arithmetic; `>>` on negative numbers is the
arithmetic shift (floor), `//` is floor division of non-negative numbers.

For an in-between frame f with keyframes a < f < b: luma -> four-level pyramid -> block matching coarse to fine for (f -> a) and
(f -> b) -> per-pixel flow in 1/16 pixel -> warps of the edited keyframes and of the source lumas -> confidence from the source
only -> blend.  The constants are restated here on purpose; tests/test_propagate.py checks that ccedit_amd/propagate.py holds the same.
"""
import numpy as np

LEVELS = 4
BLOCK = 8
APRON = 4
RADIUS_COARSEST = 4
RADIUS_FINER = 2
BOX = 5
G_SCALE = 4096
G_SIGMA = 6.0


def rank_table(radius):
    """int32 [(2R+1)^2], indexed by (dy + R) * (2R + 1) + (dx + R): the candidate's place in the order (|dy| + |dx|, dy, dx)."""
    n = 2 * radius + 1
    cands = sorted(((abs(dy) + abs(dx), dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)))
    tab = np.zeros(n * n, np.int32)
    for r, (_, dy, dx) in enumerate(cands):
        tab[(dy + radius) * n + dx + radius] = r
    return tab


def g_table():
    """int32 [256]: max(1, round(4096 / (1 + (e / 6)^2)))."""
    e = np.arange(256, dtype=np.float64)
    return np.maximum(1, np.round(G_SCALE / (1.0 + (e / G_SIGMA) ** 2))).astype(np.int32)


def luma(rgb):
    """uint8 (..., 3) -> uint8 (...): (77 R + 150 G + 29 B + 128) >> 8."""
    c = rgb.astype(np.int32)
    return ((77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8).astype(np.uint8)


def pyramid(y):
    """uint8 (H, W) -> [level 0 .. 3], each coarser level the rounded 2 x 2 mean."""
    out = [y]
    for _ in range(LEVELS - 1):
        p = out[-1].astype(np.int32)
        out.append(((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2).astype(np.uint8))
    return out


def match_level(yf, yk, pred, radius, rank=None):
    """One level.  yf, yk: uint8 (h, w); pred: int (h / 8, w / 8, 2) = (dy, dx) predictions (None: zero).  -> int32 vectors (h / 8, w / 8, 2):
    per 8 x 8 block the prediction + the candidate of the minimum key SAD * 256 + rank over the 16 x 16 patch, coordinates clamped."""
    h, w = yf.shape
    nby, nbx = h // BLOCK, w // BLOCK
    rank = rank_table(radius) if rank is None else rank
    if pred is None:
        pred = np.zeros((nby, nbx, 2), np.int64)
    pred = pred.astype(np.int64)
    span = np.arange(-APRON, BLOCK + APRON)
    ry = (np.arange(nby)[:, None] * BLOCK + span[None, :])                          # (nby, 16)
    rx = (np.arange(nbx)[:, None] * BLOCK + span[None, :])                          # (nbx, 16)
    ref = yf[np.clip(ry, 0, h - 1)[:, None, :, None], np.clip(rx, 0, w - 1)[None, :, None, :]].astype(np.int32)      # (nby, nbx, 16, 16)
    yk = yk.astype(np.int32)
    best_key = np.full((nby, nbx), np.iinfo(np.int64).max, np.int64)
    best = np.zeros((nby, nbx, 2), np.int64)
    n = 2 * radius + 1
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            ky = np.clip(ry[:, None, :, None] + (pred[..., 0] + dy)[:, :, None, None], 0, h - 1)
            kx = np.clip(rx[None, :, None, :] + (pred[..., 1] + dx)[:, :, None, None], 0, w - 1)
            sad = np.abs(ref - yk[ky, kx]).sum(axis=(2, 3)).astype(np.int64)
            key = sad * 256 + int(rank[(dy + radius) * n + dx + radius])
            better = key < best_key
            best_key = np.where(better, key, best_key)
            best[better] = (dy, dx)
    return (pred + best).astype(np.int32)


def match(pyr_f, pyr_k):
    """Coarse to fine over the two pyramids -> level-0 block vectors int32 (H / 8, W / 8, 2) pointing from frame f into the keyframe."""
    vec = None
    for lv in range(LEVELS - 1, -1, -1):
        pred = None
        if vec is not None:
            nby, nbx = pyr_f[lv].shape[0] // BLOCK, pyr_f[lv].shape[1] // BLOCK
            pred = 2 * vec[np.arange(nby)[:, None] >> 1, np.arange(nbx)[None, :] >> 1]
        vec = match_level(pyr_f[lv], pyr_k[lv], pred, RADIUS_COARSEST if lv == LEVELS - 1 else RADIUS_FINER)
    return vec


def _axis_weights(n, nb):
    t = 2 * np.arange(n) - (BLOCK - 1)
    b0 = t >> 4
    return np.clip(b0, 0, nb - 1), np.clip(b0 + 1, 0, nb - 1), 16 - (t & 15), t & 15


def flow(vec, h, w):
    """Block vectors (h / 8, w / 8, 2) -> per-pixel flow int32 (h, w, 2) in 1/16 pixel: fixed-point bilinear between block centres."""
    nby, nbx = vec.shape[:2]
    y0, y1, wy0, wy1 = _axis_weights(h, nby)
    x0, x1, wx0, wx1 = _axis_weights(w, nbx)
    v = vec.astype(np.int64)
    acc = ((wy0[:, None] * wx0[None, :])[..., None] * v[y0[:, None], x0[None, :]] + (wy0[:, None] * wx1[None, :])[..., None] * v[y0[:, None], x1[None, :]]
           + (wy1[:, None] * wx0[None, :])[..., None] * v[y1[:, None], x0[None, :]] + (wy1[:, None] * wx1[None, :])[..., None] * v[y1[:, None], x1[None, :]])
    return ((acc + 8) >> 4).astype(np.int32)


def warp(img, fl):
    """img uint8 (h, w) or (h, w, C); fl int32 (h, w, 2) -> the image sampled at 16 (y, x) + flow, clamped, bilinear with 4-bit fractions."""
    h, w = img.shape[:2]
    py = np.clip(16 * np.arange(h)[:, None] + fl[..., 0], 0, 16 * (h - 1))
    px = np.clip(16 * np.arange(w)[None, :] + fl[..., 1], 0, 16 * (w - 1))
    y0, fy, x0, fx = py >> 4, py & 15, px >> 4, px & 15
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    p = img.astype(np.int64)
    ex = (lambda a: a[..., None]) if img.ndim == 3 else (lambda a: a)
    acc = (ex((16 - fy) * (16 - fx)) * p[y0, x0] + ex((16 - fy) * fx) * p[y0, x1] + ex(fy * (16 - fx)) * p[y1, x0] + ex(fy * fx) * p[y1, x1])
    return ((acc + 128) >> 8).astype(np.uint8)


def box_error(wy, yf):
    """min(255, (5 x 5 edge-replicated box sum of |wy - yf| + 12) // 25) -> int32 (h, w)."""
    d = np.abs(wy.astype(np.int32) - yf.astype(np.int32))
    r = BOX // 2
    p = np.pad(d, r, mode="edge")
    h, w = d.shape
    s = sum(p[i:i + h, j:j + w] for i in range(BOX) for j in range(BOX))
    return np.minimum(255, (s + 12) // 25).astype(np.int32)


def blend(wa_img, wb_img, ea, eb, dist_a, dist_b, g=None):
    """w_a = dist_a g(e_a), w_b = dist_b g(e_b) (dist_a = b - f, dist_b = f - a); (w_a A + w_b B + (w_a + w_b) // 2) // (w_a + w_b)."""
    g = g_table() if g is None else g
    wa = (dist_a * g[ea].astype(np.int64))[..., None]
    wb = (dist_b * g[eb].astype(np.int64))[..., None]
    return ((wa * wa_img.astype(np.int64) + wb * wb_img.astype(np.int64) + (wa + wb) // 2) // (wa + wb)).astype(np.uint8)


def propagate_frame(s_f, s_a, s_b, e_a, e_b, dist_a, dist_b):
    """One in-between frame.  s_*: source frames, e_*: edited keyframes, uint8 (H, W, 3); dist_a = b - f, dist_b = f - a."""
    yf, ya, yb = luma(s_f), luma(s_a), luma(s_b)
    pf, pa, pb = pyramid(yf), pyramid(ya), pyramid(yb)
    h, w = yf.shape
    fa, fb = flow(match(pf, pa), h, w), flow(match(pf, pb), h, w)
    ea = box_error(warp(ya, fa), yf)
    eb = box_error(warp(yb, fb), yf)
    return blend(warp(e_a, fa), warp(e_b, fb), ea, eb, dist_a, dist_b)


def crossfade(e_a, e_b, dist_a, dist_b):
    """The plain integer cross-fade of the two keyframes: what a static scene must give."""
    d = dist_a + dist_b
    return ((dist_a * e_a.astype(np.int64) + dist_b * e_b.astype(np.int64) + d // 2) // d).astype(np.uint8)


def propagate_clip(source, key_index, edited, masks=None):
    """source uint8 (F, H, W, 3); key_index strictly increasing frame numbers (N,); edited uint8 (N, H, W, 3); masks uint8 (F, H, W) or
    None (>= 128 = edit).  -> uint8 (key_index[-1] - key_index[0] + 1, H, W, 3): keyframes as given, in-between frames propagated and,
    with masks, the source put back where a frame's own mask is clear."""
    key_index = [int(k) for k in key_index]
    first = key_index[0]
    out = np.zeros((key_index[-1] - first + 1,) + source.shape[1:], np.uint8)
    for n, k in enumerate(key_index):
        out[k - first] = edited[n]
    for n in range(len(key_index) - 1):
        a, b = key_index[n], key_index[n + 1]
        for f in range(a + 1, b):
            o = propagate_frame(source[f], source[a], source[b], edited[n], edited[n + 1], b - f, f - a)
            if masks is not None:
                o = np.where((masks[f] >= 128)[..., None], o, source[f])
            out[f - first] = o
    return out
