"""tests/_norm_ref.py pinned without a GPU, so that a wrong reference or a blind input cannot hide a wrong kernel.

1. The dispatch literals of norm.hip are the ones the case table was laid out for, and the Python copy of the dispatch sends every
   case to the arm it is meant for (a retune fails here, not silently on the GPU).
2. On every case of tests/test_norm_gpu.py the loop reference equals float64 F.group_norm / F.layer_norm to 1e-12.
3. The harness passes on every case with an emulated launch in the GPU's place (the result by vectorised float64 moments, rounded to
   bf16), and refuses a spoiled one.  This says nothing about the kernels.
4. A defect table in the manner of tests/test_attn_ref.py: the emulation with ONE mistake — statistics of the neighbouring group for
   the second part of a granule that straddles two groups, of the neighbouring pixel / clip / frame, a count of cpg (T +- 1), eps
   dropped, gamma / beta shifted by one granule, SiLU missing, the odd last row of a LayerNorm wave normalised with the previous
   row's statistics, dst_off ignored — misses the GPU limit by at least 4x on every structured case of the form it belongs to.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _norm_ref as R  # noqa: E402
from _norm_ref import BF, CASES, EPS, Case, check_case, inner, measure, predict, prepare  # noqa: E402


def test_dispatch_literals_are_the_ones_the_cases_were_laid_out_for():
    assert R.thresholds() == R.DESIGNED_FOR


@pytest.mark.parametrize("case", CASES, ids=lambda cs: cs.name)
def test_case_reaches_its_arm(case: Case):
    assert len(case.arms) == len(case.policies)
    for v in range(len(case.policies)):
        assert predict(case, v) == case.arms[v]


def test_every_arm_has_a_case():
    reached = {lb for cs in CASES for arm in cs.arms for lb in arm}
    want = ({"gn_spatial_onepass_kernel", "gn_temporal_flat_kernel<17>", "gn_temporal_flat_kernel<20>", "gn_temporal_kernel",
             "gn_temporal_stats_kernel", "gn_temporal_apply_kernel", "gn_spatial_apply_flat_kernel RS=1", "gn_spatial_apply_flat_kernel RS=8"}
            | {f"gn_spatial_apply_kernel<{n}>" for n in (1, 2, 3, 4, 5)} | {f"gn_temporal_cached_kernel nsl={n}" for n in (1, 2, 4)}
            | {f"{k}<{n}> rpw={r}" for k in ("layernorm_kernel", "row_stats_kernel") for n, r in ((3, 2), (2, 4), (1, 8), (1, 1), (2, 1), (3, 1))})
    assert want <= reached, want - reached


def test_c960_takes_the_cached_arm_at_the_flat_arms_size():
    """320 threads are not a whole number of 120-granule pixels: before the dispatch asked for 320 % (C / 8) == 0 this size went to
    gn_temporal_flat_kernel, whose threads 240..319 then normalised a pixel of the next workgroup with statistics nobody wrote."""
    case = next(cs for cs in CASES if cs.name.startswith("temporal-cached-c960"))
    th = R.thresholds()
    assert case.dims["b"] * case.dims["hw"] * (960 >> 3) >= th["flat_arm"][2] * th["flat_threads"][0] and 960 % th["flat_arm"][0] == 0
    assert predict(case) == ["gn_temporal_cached_kernel nsl=2"]


# ------------------------------------------------------------------------------------------
# float64 torch on the same inputs
# ------------------------------------------------------------------------------------------
def _torch_reference(case: Case, p):
    x = torch.from_numpy(p.x64)
    c, d = case.c, case.dims
    g, b = inner(p.gbuf, (c,)).double(), inner(p.bbuf, (c,)).double()
    if case.op == "ln":
        var, mean = torch.var_mean(x, dim=1, unbiased=False)
        return [F.layer_norm(x, (c,), g, b, EPS).numpy(), torch.stack([mean, (var + EPS).rsqrt()], dim=1).numpy()]
    if case.op == "gs":
        y = F.group_norm(x.permute(0, 2, 1), 32, g, b, EPS).permute(0, 2, 1)
    else:
        t = d["t"] if case.op == "gt" else sum(d["shards"])
        xp = x.reshape(d["b"], t, d["hw"], c).permute(0, 2, 3, 1).reshape(d["b"] * d["hw"], c, t)
        y = F.group_norm(xp, 32, g, b, EPS).reshape(d["b"], d["hw"], c, t).permute(0, 3, 1, 2).reshape(d["b"] * t, d["hw"], c)
    return [(F.silu(y) if case.silu else y).numpy()]


# ------------------------------------------------------------------------------------------
# the emulated launch, with or without one mistake
# ------------------------------------------------------------------------------------------
def _ln_tail_rows(rows, rpw):
    """Rows that a wave of layernorm_kernel handles alone (`two == false`): the last row of a wave with an odd row count."""
    r = np.arange(rows)
    last = np.minimum((r // rpw + 1) * rpw, rows) - 1
    return (r == last) & ((r - r // rpw * rpw) % 2 == 0)


def _sums(p):
    """(sum, sum of squares) per statistics block of the whole input, computed once per case."""
    if getattr(p, "_sums", None) is None:
        case, c, d = p.case, p.case.c, p.case.dims
        cpg = max(c // 32, 1)
        if case.op == "ln":
            p._sums = p.x64.sum(1), np.einsum("rc,rc->r", p.x64, p.x64)
        elif case.op == "gs":
            xg = p.x64.reshape(d["frames"], d["hw"], 32, cpg)
            p._sums = xg.sum((1, 3)), np.einsum("npgc,npgc->ng", xg, xg)
        else:
            xg = p.x64.reshape(d["b"], -1, d["hw"], 32, cpg)
            p._sums = xg.sum((1, 4)), np.einsum("btpgc,btpgc->bpg", xg, xg)
    return p._sums


def _values(p, defect=None, sel=None):
    """The outputs of the case in float64 from raw moments, vectorised, with at most one mistake.  sel: indices along the pixel axis
    (temporal) or the row axis (LayerNorm) — the statistics are those of the whole input either way, so this is the full result
    restricted to `sel`."""
    case, c, d = p.case, p.case.c, p.case.dims
    cpg = max(c // 32, 1)                                               # (LayerNorm has no groups)
    gamma, beta = inner(p.gbuf, (c,)).double().numpy(), inner(p.bbuf, (c,)).double().numpy()
    if defect == "affine+8":
        gamma, beta = np.roll(gamma, 8), np.roll(beta, 8)
    eps = 0.0 if defect == "eps" else EPS
    silu = case.silu and defect != "nosilu"
    chan = np.arange(c)
    grp = chan // cpg
    if defect in ("group+1", "group-1"):
        first = (chan // 8 * 8) // cpg                                  # the first group of the channel's 16-byte granule
        wrong = grp + (1 if defect == "group+1" else -1)
        grp = np.where(grp != first, np.where(wrong > 31, grp - 1, wrong), grp)
    sel = slice(None) if sel is None else sel

    def moments(n):
        s1, s2 = _sums(p)
        mean = s1 / n
        with np.errstate(divide="ignore"):
            return mean, 1.0 / np.sqrt(np.maximum(s2 / n - mean * mean, 0.0) + eps)

    def finish(y):
        with np.errstate(invalid="ignore", over="ignore"):
            return y / (1.0 + np.exp(-y)) if silu else y

    def shifted(a, axis):
        if defect and defect[:-2] in ("pixel", "clip", "frame") and axis == dict(pixel=1, clip=0, frame=0)[defect[:-2]]:
            return np.roll(a, -1 if defect.endswith("+1") else 1, axis=axis)
        return a

    with np.errstate(invalid="ignore"):
        if case.op == "ln":
            mean, rstd = moments(c)
            if defect == "partner":
                tail = _ln_tail_rows(d["rows"], int(predict(case)[0].split("rpw=")[1]))
                mean, rstd = np.where(tail, np.roll(mean, 1), mean), np.where(tail, np.roll(rstd, 1), rstd)
            mean, rstd = mean[sel], rstd[sel]
            return [(p.x64[sel] - mean[:, None]) * (rstd[:, None] * gamma) + beta, np.stack([mean, rstd], axis=1)]
        if case.op == "gs":
            mean, rstd = moments(cpg * d["hw"])
            mean, rstd = shifted(mean, 0), shifted(rstd, 0)
            return [finish((p.x64 - mean[:, None, grp]) * (rstd[:, None, grp] * gamma) + beta)]
        t = d["t"] if case.op == "gt" else sum(d["shards"])
        x = p.x64.reshape(d["b"], t, d["hw"], c)[:, :, sel]
        mean, rstd = moments(cpg * (t + dict(zip(("count+1", "count-1"), (1, -1))).get(defect, 0)))
        mean, rstd = shifted(shifted(mean, 0), 1)[:, sel], shifted(shifted(rstd, 0), 1)[:, sel]
        return [finish((x - mean[:, None, :, grp]) * (rstd[:, None, :, grp] * gamma) + beta).reshape(d["b"] * t, -1, c)]


def emulate(p, defect=None):
    """The output buffers as a launch would leave them: `_values` rounded to bf16 (row_stats: fp32)."""
    case, d = p.case, p.case.dims
    results = _values(p, defect)
    bufs = []
    if case.op == "gt2":
        off = 0 if defect == "dst_off0" else d["dst_off"]
        for out, ys in zip(p.outs, R.shard_frames(case, results[0])):
            buf = out.buf.clone()
            inner(buf.view(BF), out.shape)[:, off:off + ys.shape[1]] = torch.from_numpy(np.ascontiguousarray(ys)).to(BF)
            bufs.append(buf)
        return bufs
    for out, y in zip(p.outs, results):
        buf = out.buf.clone()
        inner(buf.view(BF if out.kind == "bf16" else torch.float32), out.shape).copy_(torch.from_numpy(y))
        bufs.append(buf)
    return bufs


def miss(p, defect):
    """error / limit of the emulation with one mistake, the harness's own measure.  The large temporal and LayerNorm cases are
    measured on their first and last pixels / rows only (a lower bound of the maximum over all of them)."""
    case, d = p.case, p.case.dims
    n = d["hw"] if case.op == "gt" else d.get("rows", 0)
    if case.op not in ("gt", "ln") or n <= 128:
        return max(measure(out, buf)[0] for out, buf in zip(p.outs, emulate(p, defect)))
    sel = np.r_[0:64, n - 64:n]
    got = _values(p, defect, sel)
    ratios = []
    for out, y in zip(p.outs, got):
        ref = out.ref[:, sel] if case.op == "gt" else out.ref[sel]
        part = R.Out(out.kind, ref.shape, ref, np.ones(ref.shape, dtype=bool))
        inner(part.buf.view(BF if out.kind == "bf16" else torch.float32), ref.shape).copy_(torch.from_numpy(np.ascontiguousarray(y)))
        ratio, err, lim, _ = measure(part, part.buf)
        ratios.append(ratio if out.kind != "bf16" else err / R.tolerance(out.ref))        # the limit is that of the whole output
    return max(ratios)


def defects_of(case: Case):
    """The mistakes that the form of the case can make."""
    d, cpg = case.dims, case.c // 32
    out = ["eps"] + (["affine+8"] if case.c > 8 else [])
    if case.op == "ln":
        rpw = int(predict(case)[0].split("rpw=")[1])
        return out + (["partner"] if _ln_tail_rows(d["rows"], rpw).any() else [])
    out += ["group+1", "group-1"] if cpg % 8 else []
    out += ["nosilu"] if case.silu else []
    if case.op == "gs":
        return out + ["frame+1", "frame-1"]
    t = d["t"] if case.op == "gt" else sum(d["shards"])
    out += ["pixel+1", "pixel-1", "count+1"] + (["count-1"] if t > 1 else []) + (["clip+1", "clip-1"] if d["b"] > 1 else [])
    return out + (["dst_off0"] if case.op == "gt2" else [])


def test_defect_table_covers_every_form():
    structured = [cs for cs in CASES if cs.gen == "structured"]
    seen = {(cs.op, df) for cs in structured for df in defects_of(cs)}
    for op, want in (("gt", "group+1 group-1 pixel+1 pixel-1 clip+1 clip-1 count+1 count-1 eps affine+8 nosilu"),
                     ("gt2", "group+1 group-1 pixel+1 pixel-1 clip+1 clip-1 count+1 count-1 eps affine+8 nosilu dst_off0"),
                     ("gs", "group+1 group-1 frame+1 frame-1 eps affine+8 nosilu"), ("ln", "partner eps affine+8")):
        assert {(op, df) for df in want.split()} <= seen
    # the straddling-granule logic is one function (group_split of norm.hip) that four kernels call, each with its own source of
    # statistics: each has a case with cpg % 8 != 0
    straddle = {arm[-1].split(" ")[0].split("<")[0] for cs in structured if (cs.c // 32) % 8 for arm in cs.arms}
    assert {"gn_temporal_flat_kernel", "gn_temporal_cached_kernel", "gn_spatial_apply_flat_kernel", "gn_spatial_apply_kernel"} <= straddle


@pytest.mark.parametrize("case", CASES, ids=lambda cs: cs.name)
def test_reference_harness_and_defects(case: Case):
    """One reference per case, shared by: float64 torch (1e-12), the harness on an emulated launch, the defect table."""
    p = prepare(case.name)
    for out, tref in zip(p.outs if case.op != "gt2" else [None], _torch_reference(case, p)):
        ref = out.ref if out is not None else np.concatenate([o.ref[:, case.dims["dst_off"]:-1] for o in p.outs], axis=1).reshape(tref.shape)
        assert float(np.abs(ref - tref).max()) <= 1e-12, float(np.abs(ref - tref).max())

    clean = emulate(p)

    def launch(pp):
        return [b.clone() for b in clean], [b.clone() for b in pp.inputs()], predict(case, 0)
    report = check_case(case, 0, launch, log=lambda s: None)
    unspoiled = max(err / lim for _, err, lim in report)
    if case.gen != "structured":
        return
    for defect in defects_of(case):
        ratio = miss(p, defect)
        print(f"[norm-defect] {case.name}: {defect} misses the limit by {ratio:.1f}x (unspoiled: {unspoiled:.2f}x)")
        assert ratio >= 4.0, f"{case.name}: the mistake '{defect}' moves the result by only {ratio:.2f} x the limit: the case would not notice it"


@pytest.mark.parametrize("spoil,message", [("guard", "outside the addressed set"), ("halo", "outside the addressed set"), ("nan", "non-finite"),
                                           ("label", "predicted"), ("input", "the launch changed input 0"), ("rerun", "second launch")])
def test_harness_refuses_a_spoiled_launch(spoil, message):
    case = next(cs for cs in CASES if cs.name == ("temporal-sharded-c320-off1" if spoil == "halo" else "layernorm-c520-3"))
    calls = []

    def launch(p):
        bufs, inputs, labels = emulate(p), [b.clone() for b in p.inputs()], predict(case)
        calls.append(1)
        if spoil == "guard":
            bufs[0][R.GUARD - 1] = 0
        elif spoil == "halo":
            inner(bufs[1], p.outs[1].shape)[0, 0, 0, 0] = 0          # a halo frame in front of the shard's own
        elif spoil == "nan":
            inner(bufs[0].view(BF), p.outs[0].shape)[0, 0] = float("nan")
        elif spoil == "label":
            labels[0] = "layernorm_kernel<1> rpw=1"
        elif spoil == "input":
            inputs[0][R.GUARD] = 0.0
        elif spoil == "rerun" and len(calls) == 2:
            bufs[0][R.GUARD] += 1
        return bufs, inputs, labels

    with pytest.raises(AssertionError, match=message):
        check_case(case, 0, launch, log=lambda s: None)
