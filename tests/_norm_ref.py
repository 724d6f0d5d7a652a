"""One float64 reference of the normalisation kernels of ccedit_amd/csrc/norm.hip, inputs whose statistics differ wherever a kernel
could confuse them, the case table of tests/test_norm_gpu.py and its harness (helper; no tests in here).

Reference.  `gn_spatial`, `gn_temporal`, `layernorm` and `row_stats` are indexed loops over (frame | clip, pixel, group) or rows in
numpy float64: the statistics of one block, then the block's values.  No F.group_norm, no reshape / permute that a layout mistake
could share with the code under test.  They return the value before bf16 rounding.

Inputs.  x = mu + sigma * randn, rounded to bf16, with
  * mu of opposite sign in adjacent groups (|mu| = 8 ... 17 sigma: >= 16 sigma apart), 3 sigma or more apart in adjacent pixels and
    6 sigma apart in adjacent clips (temporal), 3 sigma or more apart in adjacent frames (spatial) and 8 sigma or more apart in
    adjacent rows (LayerNorm): statistics taken from a neighbour move the normalised value by several units;
  * a ramp over the frames of a clip (temporal): a wrong T or frame stride changes both moments;
  * "quiet" blocks (mu = 0 — rows: 2^-7 —, sigma = 2^-9: variance 3.8e-6 against eps = 1e-5) spread over groups, pixels, frames and
    rows: a dropped eps doubles their output;
  * gamma in [0.5, 1.5], beta in [-1, 1], independent per channel: a channel index off by one granule moves the output by O(1).
The `offset` inputs are the existing 48 + 0.25 * randn of test_groupnorm_spatial_onepass_large_mean (|mean| = 192 std).

Harness (`check_case`).  Every operand is a 16-byte aligned view into a longer buffer: bf16 / fp32 NaN around the inputs, the bit
pattern 0x5A5A over the whole output buffers.  After the launch: the kernel label is the predicted one, the addressed outputs are
finite and within 2^-6 max|ref| + 1e-3 of the reference (the limit of the norm tests of tests/test_ops_gpu.py; row_stats: 1e-5
relative), everything else in the output buffers still holds the pattern, the inputs are unchanged bit for bit, and — for the arms
with a fixed summation order — a second launch gives the same bits.

Arm prediction (`predict`).  The dispatch arithmetic of norm.hip restated in Python, with every threshold READ from the literals of
norm.hip (`thresholds`): a retune that moves a case to another arm fails tests/test_norm_ref.py on the CPU.

What the arms share.  The kernels of norm.hip are assembled from one copy of each building block: the group boundary inside a
16-byte granule (`group_split`, behind every arm that meets a straddling granule: gn_temporal_flat, gn_temporal_cached,
gn_spatial_apply, gn_spatial_apply_flat), the affine coefficients (`affine_channel`, `affine_two_groups`), the multiply-add + SiLU +
store (`affine_store`), the temporal sweeps (`gt_stats_sweep`, `gt_affine`, `gt_apply_sweep`: gn_temporal_kernel and its sharded
halves) and the two-row LayerNorm statistics (`ln_two_row_stats`: layernorm_kernel and row_stats_kernel).  A mistake in one of
them shows on every arm that calls it; the cases still reach every arm, because each arm keeps its own mapping and source of
statistics.  The rows-per-wave loop is read from both LayerNorm entry points, which share only `ln_launch` (grid, template arm, label).
"""
import math
import os
import re
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np
import torch

BF = torch.bfloat16
OUT_FILL = 0x5A5A                     # bf16 1.7e16; as fp32 (0x5A5A5A5A) 1.5e16: finite, and no result looks like it
GUARD = 64                            # elements before and after every view (a multiple of 8: the views stay 16-byte aligned)
EPS = 1e-5
QUIET_SIGMA = 2.0 ** -9

NORM_HIP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ccedit_amd", "csrc", "norm.hip")


# ------------------------------------------------------------------------------------------
# the float64 reference
# ------------------------------------------------------------------------------------------
def _silu(v):
    return v / (1.0 + np.exp(-v))


def _block(blk, gamma, beta, eps):
    """One statistics block [..., channels of the group]: mean, variance from squared deviations, affine."""
    n = blk.size
    mean = blk.sum() / n
    d = blk - mean
    var = (d * d).sum() / n
    return d * (gamma / math.sqrt(var + eps)) + beta


def gn_spatial(x, gamma, beta, eps, silu):
    """x [frames, hw, C] float64 -> GroupNorm(32) over (hw, C / 32) of every frame (+ SiLU)."""
    frames, hw, c = x.shape
    cpg = c // 32
    out = np.empty_like(x)
    for n in range(frames):
        for g in range(32):
            ch = slice(g * cpg, (g + 1) * cpg)
            out[n, :, ch] = _block(x[n, :, ch], gamma[ch], beta[ch], eps)
    return _silu(out) if silu else out


def gn_temporal(x, b, t, gamma, beta, eps, silu):
    """x [b * t, hw, C] float64 (frames outermost, clip-major) -> GroupNorm(32) over (t, C / 32) at every (clip, pixel) (+ SiLU)."""
    frames, hw, c = x.shape
    assert frames == b * t
    cpg = c // 32
    out = np.empty_like(x)
    for clip in range(b):
        fr = slice(clip * t, (clip + 1) * t)
        for p in range(hw):
            for g in range(32):
                ch = slice(g * cpg, (g + 1) * cpg)
                out[fr, p, ch] = _block(x[fr, p, ch], gamma[ch], beta[ch], eps)
    return _silu(out) if silu else out


def layernorm(x, gamma, beta, eps):
    """x [rows, C] float64 -> LayerNorm over C."""
    out = np.empty_like(x)
    for r in range(x.shape[0]):
        out[r] = _block(x[r], gamma, beta, eps)
    return out


def row_stats(x, eps):
    """x [rows, C] float64 -> [rows, 2]: mean, 1 / sqrt(var + eps)."""
    out = np.empty((x.shape[0], 2))
    for r in range(x.shape[0]):
        mean = x[r].sum() / x.shape[1]
        d = x[r] - mean
        out[r] = mean, 1.0 / math.sqrt((d * d).sum() / x.shape[1] + eps)
    return out


# ------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------
def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def affine(c, seed):
    """gamma in [0.5, 1.5], beta in [-1, 1]: fp32, independent per channel."""
    g = torch.Generator().manual_seed(seed)
    return 0.5 + torch.rand(c, generator=g), -1.0 + 2.0 * torch.rand(c, generator=g)


def _per_channel(a, cpg):
    return a.repeat_interleave(cpg, dim=-1)


def temporal_input(b, t, hw, c, seed):
    """[b * t, hw, c] bf16.  mu[clip, pixel, group] = (-1)^group * (8 + 3 * ((pixel + 2 clip + group // 2) % 4)), sigma = 1, plus a
    ramp of 2 / t per frame; quiet blocks where (7 pixel + group + 3 clip) % 11 == 0."""
    cpg = c // 32
    clip, pix, grp = torch.arange(b)[:, None, None], torch.arange(hw)[None, :, None], torch.arange(32)[None, None, :]
    mu = torch.where(grp % 2 == 0, 1.0, -1.0) * (8.0 + 3.0 * ((pix + 2 * clip + grp // 2) % 4))
    quiet = (7 * pix + grp + 3 * clip) % 11 == 0
    mu = torch.where(quiet, 0.0, mu)
    sigma = torch.where(quiet, QUIET_SIGMA, 1.0)
    ramp = torch.where(quiet, 0.0, 2.0 / t)
    x = _randn((b, t, hw, c), seed)
    x *= _per_channel(sigma, cpg)[:, None]
    x += _per_channel(mu, cpg)[:, None]
    x += _per_channel(ramp, cpg)[:, None] * torch.arange(t, dtype=torch.float32)[None, :, None, None]
    return x.to(BF).reshape(b * t, hw, c)


def spatial_input(frames, hw, c, seed):
    """[frames, hw, c] bf16.  mu[frame, group] = (-1)^group * (8 + 3 * ((frame + group // 2) % 4)), sigma = 1; quiet blocks where
    (3 frame + group) % 8 == 5."""
    cpg = c // 32
    fr, grp = torch.arange(frames)[:, None], torch.arange(32)[None, :]
    mu = torch.where(grp % 2 == 0, 1.0, -1.0) * (8.0 + 3.0 * ((fr + grp // 2) % 4))
    quiet = (3 * fr + grp) % 8 == 5
    mu = torch.where(quiet, 0.0, mu)
    sigma = torch.where(quiet, QUIET_SIGMA, 1.0)
    x = _randn((frames, hw, c), seed)
    x *= _per_channel(sigma, cpg)[:, None]
    x += _per_channel(mu, cpg)[:, None]
    return x.to(BF)


def rows_input(rows, c, seed):
    """[rows, c] bf16.  mu[row] = (-1)^row * (4 + 3 * (row % 3)), sigma = 1; quiet rows where row % 5 == 2, with mu = 2^-7 (four of
    their sigmas) and not 0: row_stats is held to 1e-5 RELATIVE on the mean, which the rounding of any fp32 sum misses once the
    mean cancels (an fp32 emulation of row_stats_kernel's summation order with mu = 0: 1 - 2 rows of 26000 with a mean of 9e-8 from
    values of 2e-3, absolute error 1.5e-12, relative 1.6e-5 ... 3.1e-5)."""
    r = torch.arange(rows)[:, None]
    quiet = r % 5 == 2
    mu = torch.where(quiet, 4.0 * QUIET_SIGMA, torch.where(r % 2 == 0, 1.0, -1.0) * (4.0 + 3.0 * (r % 3)))
    x = _randn((rows, c), seed)
    x *= torch.where(quiet, QUIET_SIGMA, 1.0)
    x += mu
    return x.to(BF)


def offset_input(shape, seed):
    return (_randn(shape, seed) * 0.25 + 48.0).to(BF)


# ------------------------------------------------------------------------------------------
# the dispatch of norm.hip, thresholds read from its literals
# ------------------------------------------------------------------------------------------
_LITERALS = dict(
    max_cols=r"constexpr int kMaxCols = (\d+);",
    one_units=r"constexpr int kGnOneUnits = (\d+);",
    one_pass=r"if \(C % (\d+) == 0 && \(int64_t\)hw \* \(C / (\d+)\) <= (\d+) \* kGnOneUnits\)",
    cache_t=r"constexpr int kGtCacheT = (\d+);",
    flat_threads=r"constexpr int kGtFlatThreads = (\d+);",
    flat_arm=r"T <= kGtCacheT && kGtFlatThreads % \(C >> 3\) == 0 && C % (\d+) == 0 && C <= (\d+) && waves \* \(C >> 3\) >= (\d+) \* kGtFlatThreads\)",
    flat_short=r"if \(T <= (\d+)\)\s+hipLaunchKernelGGL\(gn_temporal_flat_kernel<(\d+)>",
    cached_arm=r"\} else if \(T <= kGtCacheT && \(C >> 3\) % nsl == (0)\)",
    slice_channels=r"while \(nsl < (\d+) && C / nsl > (\d+)\) nsl <<= 1;",
    gt_cols=r"constexpr int kGtCols = (\d+);",
    apply_flat=r"gn_apply_flat && \(C >> 5\) >= (\d+) && gt <= (\d+) && \(int64_t\)hw \* grid\.y >= (\d+)\)",
    apply_rs=r"int RS = (\d+) / gt;\s+RS = RS < (\d+) \? (\d+) : \(RS > (\d+) \? (\d+) : RS\);",
    apply_cols=r"const int cols = \(C / 8 \+ (\d+)\) / (\d+);\s+#define CC_GA",
    ln_rows_per_wave=r"constexpr int kLnRowsPerWave = (\d+);",
    ln_cols=r"constexpr int kLnCols = (\d+);",
    ln_rpw=r"while \(rpw > 1 && \(rows \+ 4 \* rpw - 1\) / \(4 \* rpw\) < (\d+)\) rpw >>= 1;",
)
# what the case table below was laid out for: tests/test_norm_ref.py compares
DESIGNED_FOR = dict(max_cols=(5,), one_units=(8,), one_pass=(256, 256, 256), cache_t=(20,), flat_threads=(320,), flat_arm=(320, 1280, 700),
                    flat_short=(17, 17), cached_arm=(0,), slice_channels=(32, 512), gt_cols=(3,), apply_flat=(8, 320, 4096),
                    apply_rs=(320, 1, 1, 8, 8), apply_cols=(63, 64), ln_rows_per_wave=(8,), ln_cols=(3,), ln_rpw=(4096,))


@lru_cache(maxsize=1)
def thresholds():
    """{name: tuple of ints} from the source text of norm.hip; a pattern that no longer matches is an error (the dispatch was
    rewritten: restate it in `predict`).  ln_rpw must occur twice, identically (ccedit_layernorm and ccedit_row_stats)."""
    with open(NORM_HIP) as f:
        src = f.read()
    out = {}
    for name, pat in _LITERALS.items():
        found = re.findall(pat, src)
        assert found, f"norm.hip: the dispatch literal '{name}' is not where tests/_norm_ref.py expects it"
        assert len(set(found)) == 1 and len(found) == (2 if name == "ln_rpw" else 1), (name, found)
        out[name] = tuple(int(v) for v in (found[0] if isinstance(found[0], tuple) else (found[0],)))
    return out


def _ln_arm(rows, c, th):
    rpw = th["ln_rows_per_wave"][0]
    while rpw > 1 and (rows + 4 * rpw - 1) // (4 * rpw) < th["ln_rpw"][0]:
        rpw >>= 1
    return min((c // 8 + 63) // 64, th["ln_cols"][0]), rpw


def _apply_arm(frames, hw, c, th, gn_apply_flat=1):
    gt = c >> 3
    min_cpg, max_gt, min_rows = th["apply_flat"]
    if gn_apply_flat and (c >> 5) >= min_cpg and gt <= max_gt and hw * frames >= min_rows:
        num, lo, lo_val, hi, hi_val = th["apply_rs"]
        rs = num // gt
        rs = lo_val if rs < lo else (hi_val if rs > hi else rs)
        return f"gn_spatial_apply_flat_kernel RS={rs}"
    add, div = th["apply_cols"]
    return f"gn_spatial_apply_kernel<{min((c // 8 + add) // div, th['max_cols'][0])}>"


def predict(case, variant=0):
    """The labels ccedit_last_kernel reports after each launch of the case, in launch order."""
    th = thresholds()
    pol = dict(gn_flat=1, gn_apply_flat=1)
    pol.update(dict(case.policies[variant]))
    c, d = case.c, case.dims
    if case.op == "ln":
        cols, rpw = _ln_arm(d["rows"], c, th)
        return [f"layernorm_kernel<{cols}> rpw={rpw}", f"row_stats_kernel<{cols}> rpw={rpw}"]
    if case.op == "gt2":
        return ["gn_temporal_stats_kernel", "gn_temporal_apply_kernel"]
    if case.op == "gs":
        mod, div, units = th["one_pass"]
        if d["entry"] == "internal" and c % mod == 0 and d["hw"] * (c // div) <= units * th["one_units"][0]:
            return ["gn_spatial_onepass_kernel"]
        return [_apply_arm(d["frames"], d["hw"], c, th, pol["gn_apply_flat"])]
    assert case.op == "gt"
    waves, t = d["b"] * d["hw"], d["t"]
    max_sl, sl_ch = th["slice_channels"]
    nsl = 1
    while nsl < max_sl and c // nsl > sl_ch:
        nsl <<= 1
    mod, max_c, blocks = th["flat_arm"]
    threads, cache_t = th["flat_threads"][0], th["cache_t"][0]
    if pol["gn_flat"] and t <= cache_t and threads % (c >> 3) == 0 and c % mod == 0 and c <= max_c and waves * (c >> 3) >= blocks * threads:
        short_t, short_ct = th["flat_short"]
        return [f"gn_temporal_flat_kernel<{short_ct if t <= short_t else cache_t}>"]
    if t <= cache_t and (c >> 3) % nsl == th["cached_arm"][0]:
        return [f"gn_temporal_cached_kernel nsl={nsl}"]
    return ["gn_temporal_kernel"]


# ------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    op: str                           # gt: ccedit_groupnorm_temporal; gt2: _temporal_stats + _temporal_apply; gs: spatial; ln: LayerNorm + row_stats
    c: int
    dims: dict                        # gt: b, t, hw; gt2: b, hw, shards, dst_off; gs: frames, hw, entry; ln: rows
    arms: tuple                       # per policy variant: the labels the case is meant to reach
    policies: tuple = ((),)           # policy variants, each a tuple of (switch, value); all share the inputs and the reference
    silu: bool = True
    gen: str = "structured"           # or "offset"
    seed: int = 0

    @property
    def form(self):
        return self.op if self.gen == "structured" else "offset"


_FLAT_OFF = ((), (("gn_flat", 0),))


def _cases():
    out = []

    def gt(name, c, b, hw, t, arms, **kw):
        out.append(Case(f"temporal-{name}-c{c}-b{b}x{hw}-t{t}", "gt", c, dict(b=b, hw=hw, t=t), arms, **kw))

    # flat arm and, with gn_flat = 0, the cached arm on the same large grid
    for c, b, hw, nsl, ts in ((320, 2, 2807, 1, (17, 2)), (640, 3, 937, 2, (18, 20)), (1280, 1, 1401, 4, (17, 1))):
        for t in ts:
            gt("flat", c, b, hw, t, ([f"gn_temporal_flat_kernel<{17 if t <= 17 else 20}>"], [f"gn_temporal_cached_kernel nsl={nsl}"]),
               policies=_FLAT_OFF)
    gt("below_flat", 320, 11, 509, 5, (["gn_temporal_cached_kernel nsl=1"],))               # 5599 waves: one pixel row short of 224000
    # cached arm, small grids
    gt("cached", 1280, 1, 7, 20, (["gn_temporal_cached_kernel nsl=4"],))
    gt("cached", 1536, 2, 5, 3, (["gn_temporal_cached_kernel nsl=4"],))
    gt("cached", 160, 2, 3, 4, (["gn_temporal_cached_kernel nsl=1"],))
    gt("cached", 32, 1, 6, 7, (["gn_temporal_cached_kernel nsl=1"],), silu=False)
    gt("cached", 960, 2, 950, 17, (["gn_temporal_cached_kernel nsl=2"],))                    # the flat arm's size at a width it cannot take
    # general two-sweep arm: T > 20
    for c, b, hw, t in ((320, 1, 5, 21), (320, 2, 3, 32), (1280, 2, 3, 21), (1280, 1, 5, 32), (1536, 1, 5, 21)):
        gt("general", c, b, hw, t, (["gn_temporal_kernel"],))
    # statistics of three uneven frame shards summed, applied into halo-extended buffers
    for c in (320, 1280):
        for off in (1, 2):
            out.append(Case(f"temporal-sharded-c{c}-off{off}", "gt2", c, dict(b=2, hw=6, shards=(2, 4, 3), dst_off=off),
                            (["gn_temporal_stats_kernel", "gn_temporal_apply_kernel"],)))

    def gs(name, c, frames, hw, entry, arm, **kw):
        out.append(Case(f"spatial-{name}-c{c}-{frames}x{hw}-{entry}", "gs", c, dict(frames=frames, hw=hw, entry=entry), ([arm],), **kw))

    for entry in ("internal", "producer"):
        # wave-per-row apply, one template arm each; 410 and 205 pixels: the first sizes outside the one-pass arm
        for c, frames, hw, cols in ((64, 3, 35, 1), (960, 3, 50, 2), (1536, 3, 345, 3), (1280, 3, 410, 3), (1920, 3, 33, 4), (2560, 3, 205, 5)):
            gs("rows", c, frames, hw, entry, f"gn_spatial_apply_kernel<{cols}>", silu=c != 64)
        # flat apply: 4096 and 4097 pixel rows, hw not a multiple of 4 RS; 2049 pixels: the first size outside the one-pass arm
        gs("flat", 256, 3, 2049, entry, "gn_spatial_apply_flat_kernel RS=8")
        gs("flat", 320, 2, 2048, entry, "gn_spatial_apply_flat_kernel RS=8")
        gs("flat", 320, 17, 241, entry, "gn_spatial_apply_flat_kernel RS=8")
        gs("flat", 1920, 17, 241, entry, "gn_spatial_apply_flat_kernel RS=1")
        gs("flat", 1920, 2, 2048, entry, "gn_spatial_apply_flat_kernel RS=1")
    gs("below_flat", 320, 3, 1365, "producer", "gn_spatial_apply_kernel<1>")                # 4095 pixel rows
    gs("flat", 256, 2, 2048, "producer", "gn_spatial_apply_flat_kernel RS=8", silu=False)  # (the internal entry takes one pass here)
    for c, hw in ((256, 2048), (1280, 409), (2560, 204)):                                   # the last sizes inside the one-pass arm
        gs("onepass", c, 3, hw, "internal", "gn_spatial_onepass_kernel")

    for rows, c, cols, rpw in ((32761 + 2, 1280, 3, 2), (65521 + 5, 640, 2, 4), (65521 + 6, 640, 2, 4), (131057 + 3, 320, 1, 8),
                               (3, 8, 1, 1), (3, 520, 2, 1), (3, 1536, 3, 1)):
        out.append(Case(f"layernorm-c{c}-{rows}", "ln", c, dict(rows=rows), ([f"layernorm_kernel<{cols}> rpw={rpw}", f"row_stats_kernel<{cols}> rpw={rpw}"],)))

    # |mean| = 192 std, one case per arm that forms E[x^2] - mean^2 in fp32
    off = dict(gen="offset")
    gt("offset", 320, 2, 2807, 17, (["gn_temporal_flat_kernel<17>"], ["gn_temporal_cached_kernel nsl=1"]), policies=_FLAT_OFF, **off)
    gt("offset", 1280, 2, 5, 20, (["gn_temporal_cached_kernel nsl=4"],), **off)
    gt("offset", 320, 2, 5, 21, (["gn_temporal_kernel"],), **off)
    out.append(Case("temporal-offset-sharded-c320", "gt2", 320, dict(b=2, hw=6, shards=(2, 4, 3), dst_off=1),
                    (["gn_temporal_stats_kernel", "gn_temporal_apply_kernel"],), **off))
    gs("offset", 320, 2, 2048, "internal", "gn_spatial_apply_flat_kernel RS=8", **off)
    gs("offset", 320, 3, 50, "internal", "gn_spatial_apply_kernel<1>", **off)
    for i, cs in enumerate(out):
        cs.seed = 100 + 10 * i
    assert len({cs.name for cs in out}) == len(out)
    return out


CASES = _cases()


# ------------------------------------------------------------------------------------------
# buffers
# ------------------------------------------------------------------------------------------
def guarded(values: torch.Tensor) -> torch.Tensor:
    """A 1-D buffer: GUARD NaNs, the values, GUARD NaNs (bf16 or fp32)."""
    buf = torch.full((values.numel() + 2 * GUARD,), math.nan, dtype=values.dtype)
    buf[GUARD:GUARD + values.numel()] = values.reshape(-1)
    return buf


def inner(buf: torch.Tensor, shape) -> torch.Tensor:
    """The view that `guarded` wrapped."""
    return buf[GUARD:buf.numel() - GUARD].view(shape)


@dataclass
class Out:
    kind: str                         # "bf16": int16 buffer; "f32": int32 buffer (row_stats)
    shape: tuple                      # of the view between the guards
    ref: np.ndarray                   # float64, shape `shape` (0 where not addressed)
    mask: np.ndarray                  # bool, shape `shape`: the elements the launch must write
    buf: torch.Tensor = None          # the whole buffer before the launch

    def __post_init__(self):
        n = int(np.prod(self.shape)) + 2 * GUARD
        self.buf = torch.full((n,), OUT_FILL, dtype=torch.int16) if self.kind == "bf16" else torch.full((n,), 0x5A5A5A5A, dtype=torch.int32)

    def values(self, buf):
        """float64 array of the view of a buffer after a launch."""
        v = inner(buf.view(BF if self.kind == "bf16" else torch.float32), self.shape)
        return v.double().numpy()


@dataclass
class Prepared:
    case: Case
    x64: np.ndarray                   # the whole input, float64
    xbufs: list                       # guarded bf16 buffers: one, or one per frame shard
    xshapes: list
    gbuf: torch.Tensor                # guarded fp32 gamma, beta
    bbuf: torch.Tensor
    outs: list = field(default_factory=list)

    def inputs(self):
        return self.xbufs + [self.gbuf, self.bbuf]


def make_input(case: Case) -> torch.Tensor:
    c, d = case.c, case.dims
    if case.op in ("gt", "gt2"):
        t = d["t"] if case.op == "gt" else sum(d["shards"])
        shape = (d["b"] * t, d["hw"], c)
        return offset_input(shape, case.seed) if case.gen == "offset" else temporal_input(d["b"], t, d["hw"], c, case.seed)
    if case.op == "gs":
        return offset_input((d["frames"], d["hw"], c), case.seed) if case.gen == "offset" else spatial_input(d["frames"], d["hw"], c, case.seed)
    assert case.gen == "structured"
    return rows_input(d["rows"], c, case.seed)


def reference(case: Case, x64, gamma, beta):
    """[float64 arrays]: the outputs of the case, unsharded."""
    d = case.dims
    if case.op == "gt":
        return [gn_temporal(x64, d["b"], d["t"], gamma, beta, EPS, case.silu)]
    if case.op == "gt2":
        return [gn_temporal(x64, d["b"], sum(d["shards"]), gamma, beta, EPS, case.silu)]
    if case.op == "gs":
        return [gn_spatial(x64, gamma, beta, EPS, case.silu)]
    return [layernorm(x64, gamma, beta, EPS), row_stats(x64, EPS)]


def shard_frames(case: Case, a):
    """gt2: [b * t, hw, c] -> per shard [b, ts, hw, c] (every rank holds ts consecutive frames of every clip)."""
    d = case.dims
    t = sum(d["shards"])
    a = a.reshape(d["b"], t, d["hw"], case.c)
    starts = np.cumsum((0,) + d["shards"])
    return [a[:, t0:t0 + ts] for t0, ts in zip(starts, d["shards"])]


def dst_frames(case: Case, ts):
    return ts + case.dims["dst_off"] + 1          # dst_off halo frames before the shard's own, one after


@lru_cache(maxsize=1)
def prepare(name: str) -> Prepared:
    """Inputs, reference and buffers of one case (the last case is kept: the variants of a case and the launches of the harness share
    one reference)."""
    case = next(cs for cs in CASES if cs.name == name)
    x = make_input(case)
    gamma, beta = affine(case.c, case.seed + 1)
    x64 = x.double().numpy()
    refs = reference(case, x64, gamma.double().numpy(), beta.double().numpy())
    p = Prepared(case, x64, [], [], guarded(gamma), guarded(beta))
    if case.op == "gt2":
        off = case.dims["dst_off"]
        for xs, rs in zip(shard_frames(case, x), shard_frames(case, refs[0])):
            b, ts, hw, c = xs.shape
            p.xbufs.append(guarded(xs.contiguous()))
            p.xshapes.append((b * ts, hw, c))
            ref = np.zeros((b, dst_frames(case, ts), hw, c))
            mask = np.zeros(ref.shape, dtype=bool)
            ref[:, off:off + ts] = rs
            mask[:, off:off + ts] = True
            p.outs.append(Out("bf16", ref.shape, ref, mask))
    else:
        p.xbufs.append(guarded(x))
        p.xshapes.append(tuple(x.shape))
        p.outs.append(Out("bf16", refs[0].shape, refs[0], np.ones(refs[0].shape, dtype=bool)))
        if case.op == "ln":
            p.outs.append(Out("f32", refs[1].shape, refs[1], np.ones(refs[1].shape, dtype=bool)))
    return p


# ------------------------------------------------------------------------------------------
# the harness
# ------------------------------------------------------------------------------------------
FIXED_ORDER = ("gn_spatial_onepass_kernel", "gn_temporal_flat_kernel", "gn_spatial_apply_flat_kernel", "layernorm_kernel", "row_stats_kernel")


def tolerance(ref_on_mask) -> float:
    """The limit of the norm tests of tests/test_ops_gpu.py: 2^-6 of max |ref| plus 1e-3."""
    return 2.0 ** -6 * float(np.abs(ref_on_mask).max()) + 1e-3


def measure(out: Out, buf):
    """(error / limit, error, limit, all finite) of one output buffer after a launch.  bf16: max |got - ref| against `tolerance`.
    row_stats: |got - ref| against 1e-5 |ref|, for the mean and for rstd separately."""
    got = out.values(buf)
    finite = bool(np.isfinite(got[out.mask]).all())
    if out.kind == "bf16":
        lim = tolerance(out.ref[out.mask])
        err = float(np.nan_to_num(np.abs(got - out.ref)[out.mask], nan=np.inf).max())
        return err / lim, err, lim, finite
    diff, scale = np.nan_to_num(np.abs(got - out.ref), nan=np.inf), np.abs(out.ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = float(np.where(diff == 0.0, 0.0, diff / scale).max())          # (a reference of exactly 0 admits exactly 0)
    return rel / 1e-5, rel, 1e-5, finite


def check_case(case: Case, variant: int, launch, log=print) -> list:
    """The one harness of tests/test_norm_gpu.py.  launch(prepared) runs the case once on copies of the buffers and returns
    (output buffers, input buffers in the order of Prepared.inputs(), labels), all on the CPU, as they are after the launch.
    Returns the (label, error, limit) of every output."""
    p = prepare(case.name)
    want = predict(case, variant)
    assert want == case.arms[variant], f"{case.name}: norm.hip now sends this case to {want}, it was laid out for {case.arms[variant]}"
    got_bufs, inputs_after, labels = launch(p)
    assert labels == want, f"{case.name}: ran {labels}, predicted {want}"
    report = []
    for i, (out, buf) in enumerate(zip(p.outs, got_bufs)):
        ratio, err, lim, finite = measure(out, buf)
        bits, before = inner(buf, out.shape).numpy(), inner(out.buf, out.shape).numpy()
        touched = int((bits != before)[~out.mask].sum()) + int((buf[:GUARD] != out.buf[:GUARD]).sum()) + int((buf[-GUARD:] != out.buf[-GUARD:]).sum())
        label = labels[min(i, len(labels) - 1)] if case.op == "ln" else labels[-1]
        log(f"[norm] {case.name} [{label}] output {i}: max err {err:.4g}, limit {lim:.4g}; non-finite {not finite}; guard elements changed {touched}")
        assert finite, f"{case.name}: non-finite output"
        assert err <= lim, f"{case.name}: output {i} [{label}]: max err {err:.4g} > {lim:.4g}"
        assert touched == 0, f"{case.name}: {touched} elements outside the addressed set were written"
        report.append((label, err, lim))
    for k, (after, before) in enumerate(zip(inputs_after, p.inputs())):
        as_bits = torch.int16 if before.dtype == BF else torch.int32
        assert torch.equal(after.view(as_bits), before.view(as_bits)), f"{case.name}: the launch changed input {k}"
    if all(lb.startswith(FIXED_ORDER) for lb in labels):
        again = launch(p)[0]
        assert all(torch.equal(a, b) for a, b in zip(again, got_bufs)), f"{case.name}: a second launch gave other bits"
    return report
