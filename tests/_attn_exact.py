"""Attention on a power-of-two score grid: inputs, the exact reference, the conditions and the harness of
tests/test_attn_exact_gpu.py and tests/test_attn_exact_ref.py (helper; no tests in here).

Premise.  q, k, v are small integers and the softmax scale in log2 units is exactly 1 (CCEDIT_ATTN_Q_LOG2, or
scale = float32(ln 2): fp32(scale * fp32(log2 e)) == 1.0f).  Every score is then an integer, every p = 2^(s - m) a power of two
whatever integer reference m a kernel uses, every rescale factor a power of two, and every partial sum of p * v in any order a
multiple of one quantum below 2^24 quanta: exact in fp32 under every lane map, tile order, ring depth and MFMA shape.  What is left
to a kernel is 1.0f / l, o * inv and the bf16 store; the expected value is one float64 division of two exactly known integers.

Channels of every head: the first ones, "free", carry the random part (q has `nnz` entries +-1 per row, k entries in {-1, 0, 1},
in the staircase {-1, 1}); the last ones carry structure, in this order:
    bump    q = 1 in rows i % 4 == 2, k = 10 at key 5: from the first tile on, those rows compute every other p at about 2^-10 of
            their maximum, and Lk of them make up several per cent of the denominator — what a flush of small p would lose
            (only with Lk >= 16 and Lq >= 3, not in the staircase)
    tilt    q = 1 in rows i % 4 == 1, k = 9 at the keys of the last 64-key tile (causal: of every tile but the first): those rows
            find their maximum there (only in cases with more than one key tile that are no staircase)
    shift   q = 1 in every row, k = shift + stair * (key // 64); shift = 1 unless the variant says otherwise (not 0: every channel
            has a non-zero k)
    spike   q = 1 in the spiked rows only, k = 200 at the spike keys (only in the spike variant)
At the spike keys the free channels of k are 0, so a spiked row weighs its (up to four) spike keys equally: its denominator is a
power of two, its result exact in fp32 before the store, and v there is chosen so that the result is an exact bf16 tie of either
parity.
"""
import math
from functools import lru_cache

import numpy as np
import torch

from _attn_cases import BF, Case, build, expected_arm
from _attn_ref import Rules

LN2F = 0.6931471824645996             # float32(ln 2); np.float32(LN2F) * np.float32(log2 e) == 1.0f (tests/test_attn_exact_ref.py)
SHIFT_LOW, SHIFT_HIGH, SPIKE, TILT, BUMP, BUMP_KEY = -24, 120, 200, 9, 10, 5
LIVE, DEAD = 24, 150                  # a term is live within 24 of the row maximum; every other one is >= 150 below it
REL = 2.0 ** -17                      # (32 rescale factors + 1 p + 1.0f / l and the product) * 2^-23 < 2^-17, see DESIGN.md 5.3


# ------------------------------------------------------------------------------------------------------------------ bf16 rounding
def ulp_bf16(x):
    """2^(floor(log2 x) - 7) of a positive float64 tensor."""
    _, e = torch.frexp(x)             # x = m * 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(x), e - 8)


def _round_bf16(x, how):
    a = x.abs()
    u = ulp_bf16(torch.where(a > 0, a, torch.ones_like(a)))
    n = a / u                          # exact: u is a power of two
    n = {"rne": torch.round, "trunc": torch.floor, "away": lambda t: torch.floor(t + 0.5)}[how](n)      # torch.round: half to even
    return torch.sign(x) * n * u


def bf16_rne(x):
    """float64 -> the nearest bf16 value (ties to even), as float64; no detour through fp32 (no double rounding)."""
    return _round_bf16(x, "rne")


def bound(ref):
    """2^-17 |ref| + 1/2 ulp_bf16(|ref| (1 + 2^-17)); 0 where ref == 0 (the output must be +-0 there)."""
    a = ref.abs()
    return torch.where(a > 0, REL * a + 0.5 * ulp_bf16(torch.where(a > 0, a * (1 + REL), torch.ones_like(a))), torch.zeros_like(a))


def miss(err, lim):
    """|err| / bound per element; inf where the bound is 0 and the error is not."""
    return torch.where(lim > 0, err / lim.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))


# ---------------------------------------------------------------------------------------------------------------------- the inputs
def mode_desc(case: Case, mode: str) -> dict:
    """The keywords of one launch: the case's descriptor plus the way the unit scale reaches the kernel."""
    return dict(case.desc, **({"q_log2": True} if mode == "q_log2" else {"scale": LN2F}))


def _tiles(lk):
    return (lk + 63) // 64


def uses_tilt(case: Case) -> bool:
    return case.meta["variant"] != "stair" and case.desc["lk"] > 64


def uses_bump(case: Case) -> bool:
    return case.meta["variant"] != "stair" and case.desc["lk"] >= 16 and case.desc["lq"] >= 3


def _row_index(r: Rules, n_q, n_kv):
    """Logical query index and ordinal of every q row, logical key index of every k / v row (-1: not addressed)."""
    qi, qn, kj = np.full(n_q, -1), np.full(n_q, -1), np.full(n_kv, -1)
    count = 0
    for batch in range(r.batches):
        rows = np.array(r.q_rows(batch))
        assert (qi[rows] == -1).all(), "two (batch, query) share a q row"
        qi[rows] = np.arange(r.lq)
        qn[rows] = count + np.arange(r.lq)
        count += r.lq
        rows = np.array(r.kv_rows(batch))
        assert ((kj[rows] == -1) | (kj[rows] == np.arange(r.lk))).all(), "a k / v row serves as two different keys"
        kj[rows] = np.arange(r.lk)
    return qi, qn, kj


@lru_cache(maxsize=None)
def _grid_build(name):
    case = BY_NAME[name]
    m = case.meta
    variant, nnz, vmax = m["variant"], m["nnz"], m["vmax"]
    b = build(case)                    # the layout of tests/_attn_cases.py: slices of wider, longer buffers, NaN off the read masks
    r = Rules(case.heads, case.d, **case.desc)
    d = case.d
    q, k, v = b.qbuf[:, b.qcols], b.kbuf[:, b.kcols], b.vbuf[:, b.vcols]
    qi, qn, kj = _row_index(r, q.shape[0], k.shape[0])
    qa, ka = np.flatnonzero(qi >= 0), np.flatnonzero(kj >= 0)
    bump, tilt, spike = uses_bump(case), uses_tilt(case), variant == "spike"
    nfree = d - 1 - int(bump) - int(tilt) - int(spike)
    assert nnz <= nfree
    c_bump, c_tilt, c_shift, c_spike = nfree, nfree + int(bump), nfree + int(bump) + int(tilt), d - 1      # after the free channels
    shift = {"shift": SHIFT_LOW, "high": SHIFT_HIGH}.get(variant, 1)
    stair = int(variant == "stair")
    rs = np.random.RandomState(case.seed)
    ntl = _tiles(r.lk)
    is_sk = np.isin(kj[ka], m["spike_keys"]) if spike else np.zeros(len(ka), bool)
    for h in range(case.heads):
        # q: nnz entries +-1 per row; within every block of nfree rows each free channel is used exactly nnz times
        n = qn[qa]
        perms = np.stack([rs.permutation(nfree) for _ in range(n.max() // nfree + 1)])
        qh = np.zeros((len(qa), d), np.int64)
        for t in range(nnz):
            qh[np.arange(len(qa)), perms[n // nfree, ((n % nfree) * nnz + t) % nfree]] = rs.choice([-1, 1], len(qa))
        kh = np.zeros((len(ka), d), np.int64)
        kh[:, :nfree] = rs.choice([-1, 1], (len(ka), nfree)) if stair else rs.randint(-1, 2, (len(ka), nfree))
        vh = rs.randint(-vmax, vmax + 1, (len(ka), d))
        qh[:, c_shift] = 1
        kh[:, c_shift] = shift + stair * (kj[ka] // 64)
        if bump:
            qh[:, c_bump] = qi[qa] % 4 == 2
            kh[:, c_bump] = BUMP * (kj[ka] == BUMP_KEY)
        if tilt:
            qh[:, c_tilt] = qi[qa] % 4 == 1
            kh[:, c_tilt] = TILT * (kj[ka] >= (64 if r.causal else 64 * (ntl - 1)))
        if spike:
            qh[:, c_spike] = np.isin(qi[qa], m["spike_rows"])
            kh[is_sk, c_spike] = SPIKE
            if len(m["spike_keys"]) == 4:      # (fewer: Lk < 4 — the spike keys keep their random part)
                kh[is_sk, :c_spike] = 0
                # a row that sees all four: (256 + 256 + 4 c + 2 + 0) / 4 = 128 + c + 1/2, an exact bf16 tie; the kept bit is c's parity
                ch = np.arange(d)
                sgn = np.where(ch % 4 < 2, 1, -1)
                for pos, val in enumerate((256 * sgn, 256 * sgn, (4 * (ch % 16) + 2) * sgn, 0 * ch)):
                    vh[kj[ka] == m["spike_keys"][pos]] = val
        c0 = h * d
        q[torch.from_numpy(qa), c0:c0 + d] = torch.from_numpy(qh).to(BF)
        k[torch.from_numpy(ka), c0:c0 + d] = torch.from_numpy(kh).to(BF)
        v[torch.from_numpy(ka), c0:c0 + d] = torch.from_numpy(vh).to(BF)
    return b


def grid_build(case: Case):
    """The CPU buffers of one case (cached: every caller copies before it writes)."""
    return _grid_build(case.name)


# ------------------------------------------------------------------------------------------------------------- reference, conditions
def _heads(case: Case, b):
    """(h, q [B, Lq, d], k [B, Lk, d], v [B, Lk, d], vis [Lq, Lk], out rows [B, Lq], c0) per head: float64 operands of all batches,
    gathered row by row through the descriptor's rules."""
    r = Rules(case.heads, case.d, **case.desc)
    q2, k2, v2 = b.qbuf[:, b.qcols], b.kbuf[:, b.kcols], b.vbuf[:, b.vcols]
    vis = torch.tensor([[r.visible(i, j) for j in range(r.lk)] for i in range(r.lq)]) if r.causal else torch.ones(r.lq, r.lk, dtype=torch.bool)
    qr = torch.tensor([r.q_rows(batch) for batch in range(r.batches)])
    kr = torch.tensor([r.kv_rows(batch) for batch in range(r.batches)])
    for h in range(case.heads):
        c0 = r.head_col(h)
        yield h, q2[qr, c0:c0 + r.d].double(), k2[kr, c0:c0 + r.d].double(), v2[kr, c0:c0 + r.d].double(), vis, qr, c0


class Analysis:
    """ref, written, pow2 (out-shaped tensors), spread, first_frac, last_frac, upper, lower, pow2_ties of one case."""


@lru_cache(maxsize=None)
def _analyse(name):
    """The exact reference of a case with the exactness and coverage conditions asserted on its inputs."""
    case = BY_NAME[name]
    b = grid_build(case)
    m = case.meta
    variant = m["variant"]
    lq, lk, d = case.desc["lq"], case.desc["lk"], case.d
    oshape = (b.qbuf.shape[0], case.heads * d)
    a = Analysis()
    a.ref = torch.zeros(oshape, dtype=torch.float64)
    a.written = torch.zeros(oshape, dtype=torch.bool)
    a.pow2 = torch.zeros(oshape, dtype=torch.bool)              # rows whose denominator is a power of two
    ntl = _tiles(lk)
    tile_of = torch.arange(lk) // 64
    q_rows_nz = torch.zeros(case.heads, d)
    k_live_nz = torch.zeros(case.heads, d, dtype=torch.bool)
    first_tile = last_tile = multi = 0
    a.spread = 0
    for h, q, k, v, vis, rows, c0 in _heads(case, b):
        assert all(bool((t == t.round()).all()) for t in (q, k, v)), "inputs off the integer grid"
        s = (q @ k.transpose(1, 2)).masked_fill(~vis, -math.inf)                    # [B, Lq, Lk]
        mx = s.max(dim=2, keepdim=True).values
        gap = mx - s
        live = gap <= LIVE
        assert bool((live | ~vis | (gap >= DEAD)).all()), f"{name}: a term between {LIVE} and {DEAD} below its row maximum"
        rr = torch.where(live, gap, torch.zeros_like(gap)).max(dim=2, keepdim=True).values
        w = torch.where(live, torch.exp2(rr - gap), torch.zeros_like(gap))          # integers <= 2^24
        assert (w @ v.abs()).max().item() < 2.0 ** 24, f"{name}: sums beyond 24 bits"
        den = w.sum(dim=2, keepdim=True)
        a.ref[rows, c0:c0 + d] = (w @ v) / den
        a.written[rows, c0:c0 + d] = True
        _, e = torch.frexp(den)
        a.pow2[rows, c0:c0 + d] = (den == torch.ldexp(torch.ones_like(den), e - 1)).expand(-1, -1, d)
        a.spread = max(a.spread, int(rr.max()))
        # coverage
        q_rows_nz[h] += (q != 0).sum(dim=(0, 1))
        k_live_nz[h] |= ((k != 0) & live.any(dim=1)[:, :, None]).any(dim=1).any(dim=0)
        if ntl > 1:
            tmax = torch.stack([s[:, :, tile_of == t].max(dim=2).values for t in range(ntl)], dim=2)      # [B, Lq, tiles], -inf where none visible
            seen = (tmax > -math.inf).sum(dim=2)               # visible tiles of the row (causal: a prefix)
            run = torch.cummax(tmax, dim=2).values
            first = (run == mx).int().argmax(dim=2)            # the tile that first reaches the row maximum
            many = seen > 1
            multi += int(many.sum())
            first_tile += int((many & (first == 0)).sum())
            last_tile += int((many & (first == seen - 1)).sum())
            if variant == "stair":
                assert bool(((tmax[:, :, 1:] > run[:, :, :-1]) | (tmax[:, :, 1:] == -math.inf)).all()), f"{name}: a row does not raise its maximum in every key tile"
    # every channel: non-zero in >= 8 query rows (the spike channel: in the spiked rows) and non-zero in a live key
    spike_ch = d - 1 if variant == "spike" else -1
    for h in range(case.heads):
        for c in range(d):
            need = 1 if c == spike_ch else 8
            assert q_rows_nz[h, c] >= need, f"{name}: channel {c} of head {h} is non-zero in {int(q_rows_nz[h, c])} query rows"
        assert bool(k_live_nz[h].all()), f"{name}: head {h}: a channel has no non-zero live k"
    a.first_frac = a.last_frac = None
    if multi:
        a.first_frac, a.last_frac = first_tile / multi, last_tile / multi
        assert a.last_frac >= 1 / 8, f"{name}: {a.last_frac:.3f} of the rows find their maximum in their last key tile"
        assert variant == "stair" or a.first_frac >= 1 / 8, f"{name}: {a.first_frac:.3f} of the rows find their maximum in the first key tile"
    # both halves of the bf16 interval
    rw = a.ref[a.written].abs()
    nzr = rw[rw > 0]
    pos = nzr / ulp_bf16(nzr)
    frac = pos - pos.floor()
    a.upper, a.lower = float((frac > 0.5).float().mean()), float(((frac > 0) & (frac < 0.5)).float().mean())
    ar = a.ref.abs()
    a.pow2_ties = int(((ar / ulp_bf16(ar.clamp_min(2.0 ** -60)) % 1 == 0.5) & a.pow2 & a.written).sum())      # ties the store alone decides
    # (Lk == 1: the result is v itself, nothing is rounded)
    assert lk == 1 or (a.upper >= 1 / 64 and a.lower >= 1 / 64), f"{name}: upper / lower half of the bf16 interval hold {a.upper:.4f} / {a.lower:.4f} of the outputs"
    if variant == "spike":
        arm = expected_arm(case)
        wg = 32 * arm["nw"] if arm["kernel"] in ("attn_kernel", "attn_spatial_kernel") else 32
        sr = m["spike_rows"]
        assert any(i % wg < 32 for i in sr) and any(i // 32 == (lq - 1) // 32 for i in sr), f"{name}: spiked rows miss a wave position"
        assert lq < wg or any(i % wg >= wg - 32 for i in sr), f"{name}: no spiked row in the last wave of a workgroup"
        assert len(m["spike_keys"]) < 4 or a.pow2_ties >= case.heads * d, f"{name}: the spiked rows make {a.pow2_ties} exact ties"
    return a


def analyse(case: Case) -> Analysis:
    return _analyse(case.name)


# ------------------------------------------------------------------------------------------ fp32 emulation of attn_kernel's loop
def emulate(case: Case, mode: str, defect: str = None):
    """The online loop of attention.hip in fp32: 64-key tiles, running maximum, rescale when a maximum moves, the denominator summed
    from fp32 p (d % 32 == 0) or delivered by a ones column of V through the product with bf16 p (otherwise); 1.0f / l, o * inv.
    Returns the fp32 value in front of the store as float64, in the shape of the out view.  `defect` plants one mistake."""
    b = grid_build(case)
    d, lk = case.d, case.desc["lk"]
    m = case.meta
    f32 = torch.float32
    scale = 1.0 if defect != "scale_d" or mode == "q_log2" else float(np.float32(np.float32(d ** -0.5) * np.float32(1.4426950408889634)))
    out = torch.zeros((b.qbuf.shape[0], case.heads * d), dtype=torch.float64)
    ones_col = d % 32 != 0
    for h, q, k, v, vis, rows, c0 in _heads(case, b):
        q, k, v = q.to(f32), k.to(f32), v.to(f32)
        nb, lq = q.shape[0], q.shape[1]
        if defect == "channels_32_40":
            q = q.clone()
            q[:, :, 32:40] = 0
        if defect == "causal_lt":
            vis = vis & ~torch.eye(lq, dtype=torch.bool)
        if defect == "drop_last_key":
            vis = vis.clone()
            vis[:, lk - 1] = False
        if defect == "admit_key_lk":                               # the zero page's (or the padding's) key: k = 0, v = 0
            k, v = torch.cat([k, torch.zeros(nb, 1, d)], dim=1), torch.cat([v, torch.zeros(nb, 1, d)], dim=1)
            vis = torch.cat([vis, torch.ones(lq, 1, dtype=torch.bool)], dim=1)
        s = (q @ k.transpose(1, 2)) * scale
        s = s.masked_fill(~vis, -math.inf)
        o = torch.zeros(nb, lq, d, dtype=f32)
        l = torch.zeros(nb, lq, 1, dtype=f32)
        m_run = torch.full((nb, lq, 1), -math.inf, dtype=f32)
        for t in range(_tiles(k.shape[1])):
            if defect == "skip_spike_tile" and t == m["spike_keys"][len(m["spike_keys"]) // 2] // 64:
                continue
            st, vt = s[:, :, 64 * t:64 * t + 64], v[:, 64 * t:64 * t + 64]
            m_new = torch.maximum(m_run, st.max(dim=2, keepdim=True).values)
            alpha = torch.exp2(m_run - m_new)
            alpha = torch.where(m_new == m_run, torch.ones_like(alpha), alpha)      # the maximum did not move: no rescale
            if defect == "no_rescale_by_one":
                alpha = torch.where(m_new - m_run == 1, torch.ones_like(alpha), alpha)
            l = l * alpha
            if defect == "no_rescale_last_tile":                   # channels [32 (NT - 1), d) keep their old reference
                o = torch.cat([o[:, :, :32 * ((d - 1) // 32)] * alpha, o[:, :, 32 * ((d - 1) // 32):]], dim=2)
            else:
                o = o * alpha
            m_run = m_new
            p = torch.exp2(st - m_run)
            if defect == "flush_p":
                p = torch.where(p < 2.0 ** -8, torch.zeros_like(p), p)
            l = l + (p.to(BF).to(f32) if ones_col else p).sum(dim=2, keepdim=True)
            o = o + p.to(BF).to(f32) @ vt
        if defect == "neighbour_denominator":
            l = torch.roll(l, 1, dims=1)
        out[rows, c0:c0 + d] = (o * (torch.ones((), dtype=f32) / l)).double()
    return out


# --------------------------------------------------------------------------------------------------------------------- the harness
def check_exact(case: Case, launch, stats: dict = None) -> None:
    """launch(built, desc, policy) runs the case once on copies of the buffers, with the keywords `desc` under the policy switches
    `policy`, and returns (out buffer int16, q buffer, k buffer, v buffer, kernel label), all on the CPU.  Asserted per launch (every
    mode x policy of the case): the label; for every addressed element |got - ref| <= 2^-17 |ref| + 1/2 ulp_bf16(|ref| (1 + 2^-17)),
    +-0 where ref == 0; bit equality with bf16_rne(ref) in rows whose denominator is a power of two (1.0f / l and o * inv are then
    exact, only the store rounds); everything off the written mask untouched; inputs unchanged; a second launch bit-identical; a
    spatial workgroup that holds a spiked row equal under attn_opt 1 and 0."""
    a = analyse(case)
    b = grid_build(case)
    ref, written = a.ref, a.written
    full_mask = torch.zeros(b.obuf.shape, dtype=torch.bool)
    full_mask[:, b.ocols] = written
    lim = bound(ref)
    rne = bf16_rne(ref)
    half = 0.5 * ulp_bf16(ref.abs().clamp_min(2.0 ** -60))
    by_policy = {}
    for mode in case.meta["modes"]:
        for policy in case.meta["policies"]:
            arm = expected_arm(Case(case.name, case.kernel, case.heads, case.d, mode_desc(case, mode)), policy)
            got_bits, q_after, k_after, v_after, label = launch(b, mode_desc(case, mode), policy)
            got = got_bits.view(BF)[:, b.ocols].double()
            what = f"{case.name} [{mode}{''.join(f', {k}={v}' for k, v in policy.items())}]"
            assert label == f"{arm['kernel']} d={case.d}" and arm["kernel"] == case.kernel, f"{what}: ran {label!r}, meant for {case.label!r}"
            finite = bool(torch.isfinite(got[written]).all())
            err = (got - ref).abs()
            ratio = miss(err, lim)[written]
            worst = ratio.max().item() if finite else math.inf
            nz = written & (ref != 0)
            excess = ((err - half) / ref.abs())[nz].max().item() if finite else math.inf
            differ = int((got != rne)[written].sum())
            zero_bad = int(((got_bits.view(torch.int16)[:, b.ocols] & 0x7FFF) != 0)[written & (ref == 0)].sum())
            pow2_bad = int((got != rne)[written & a.pow2].sum())
            touched = int((got_bits != b.obuf)[~full_mask].sum())
            print(f"[attn-exact] {what}: {label}; worst |err| / bound {worst:.4f}; largest (|err| - ulp/2) / |ref| {excess:.3e} "
                  f"(2^-23 = 1.19e-07); differ from bf16_rne(ref) {differ} of {int(written.sum())}; spread {a.spread}; exact ties in "
                  f"power-of-two rows {a.pow2_ties}; unaddressed output elements changed {touched}")
            if stats is not None:
                st = stats.setdefault(case.kernel, dict(launches=0, worst=0.0, excess=-math.inf, differ=0, elements=0))
                st["launches"] += 1
                st["worst"], st["excess"] = max(st["worst"], worst), max(st["excess"], excess)
                st["differ"] += differ
                st["elements"] += int(written.sum())
            assert finite, f"{what}: non-finite output"
            if worst > 1:
                bad = torch.nonzero(torch.where(written, miss(err, lim), torch.zeros_like(err)) > 1)
                i, c = bad[0].tolist()
                raise AssertionError(f"{what}: {len(bad)} elements outside the bound, worst {worst:.4g} x; first at out row {i}, column {c}: "
                                     f"got {got[i, c].item()!r}, ref {ref[i, c].item()!r}; rows {sorted(set(bad[:, 0].tolist()))[:12]}, "
                                     f"columns {sorted(set(bad[:, 1].tolist()))[:12]}")
            assert zero_bad == 0, f"{what}: {zero_bad} elements with ref == 0 are not +-0"
            assert pow2_bad == 0, f"{what}: {pow2_bad} elements of rows with a power-of-two denominator differ from bf16_rne(ref)"
            assert touched == 0, f"{what}: {touched} output elements outside the addressed set were written"
            for nm, after, before in (("q", q_after, b.qbuf), ("k", k_after, b.kbuf), ("v", v_after, b.vbuf)):
                assert torch.equal(after.view(torch.int16), before.view(torch.int16)), f"{what}: the launch changed {nm}"
            again = launch(b, mode_desc(case, mode), policy)[0]
            assert torch.equal(again, got_bits), f"{what}: a second launch gave other bits"
            by_policy[(mode, tuple(sorted(policy.items())))] = got_bits
    if case.kernel == "attn_spatial_kernel" and case.meta["variant"] == "spike":
        # the spiked rows' workgroups (256 query rows) overflowed the optimistic pass and ran again with the tracked reference
        r = Rules(case.heads, case.d, **case.desc)
        for (mode, pol), bits in by_policy.items():
            other = dict(pol)
            if other.get("attn_opt", 1) == 0:
                continue
            other["attn_opt"] = 0
            trk = by_policy[(mode, tuple(sorted(other.items())))]
            for batch in range(r.batches):
                for i in case.meta["spike_rows"]:
                    rows = torch.tensor([r.q_row(batch, x) for x in range(i // 256 * 256, min(i // 256 * 256 + 256, r.lq))])
                    assert torch.equal(bits[rows], trk[rows]), f"{case.name} [{mode}]: the workgroup of spiked row {i} differs from attn_opt = 0"


def fake_launch(case: Case, value_of):
    """A launch for check_exact without a GPU: value_of(mode) gives the float64 values of the out view, stored as bf16 (they are bf16
    numbers already, or the conversion rounds to nearest even)."""
    a = analyse(case)

    def launch(b, desc, policy):
        mode = "q_log2" if desc.get("q_log2") else "scale"
        out = b.obuf.clone()
        view = out.view(BF)[:, b.ocols]
        view[a.written] = value_of(mode)[a.written].to(BF)
        return out, b.qbuf, b.kbuf, b.vbuf, f"{expected_arm(Case(case.name, case.kernel, case.heads, case.d, desc), policy)['kernel']} d={case.d}"
    return launch


# ----------------------------------------------------------------------------------------------------------------------- the cases
def _temporal(tl, tg, hw, clips=2):
    return dict(batches=clips * hw, lq=tl, lk=tg, q_inner=hw, q_outer_rows=tl * hw, q_inner_rows=1, q_seq_rows=hw,
                kv_inner=hw, kv_outer_rows=tg * hw, kv_inner_rows=1, kv_seq_rows=hw)


def _spike_sets(desc, arm):
    """Spiked rows: first wave of a workgroup, its last wave, the last (ragged) 32-row tile.  Spike keys: first key tile, a middle
    one, key Lk - 1 and one more (four keys weigh 1/4 each: a power-of-two denominator) — not the first tile on the spatial kernel,
    whose optimistic pass must overflow.  causal: the spike keys are the diagonal of the spiked rows."""
    lq, lk = desc["lq"], desc["lk"]
    wg = 32 * arm["nw"] if arm["kernel"] in ("attn_kernel", "attn_spatial_kernel") else 32
    if desc.get("causal"):
        rows = sorted({min(6, lq - 1), min(40, lq - 1), wg - 3 if wg - 3 < lq else lq // 2, lq - 1})      # (not 5: the bump key)
        return rows, rows
    rows = sorted({min(5, lq - 1), wg - 3 if wg - 3 < lq else lq // 2, lq - 1}) if lq >= 8 else sorted({0, min(1, lq - 1)})      # (row 2: bump)
    nt = _tiles(lk)
    cand = [7, 64 * (nt // 2) + 3, lk - 1, 65, 64 * (nt - 1) + 1, 130, 2, 1, 0, 3]
    lo = 64 if arm["kernel"] == "attn_spatial_kernel" else 0
    keys = []
    for j in cand:
        if lo <= j < lk and j not in keys and len(keys) < 4:
            keys.append(j)
    return rows, sorted(keys)


def _add(out, shape, kernel, heads, d, desc, variants, modes, policies=({},), nnz=4):
    for variant in variants:
        if variant == "stair" and (desc["lk"] <= 128 or desc.get("causal")):
            continue          # (causal: the tile on the diagonal holds too few keys for every row to find a new maximum there)
        cs = Case(f"{shape}-{variant}", kernel, heads, d, dict(desc),
                  meta=dict(variant=variant, nnz=2 if variant == "stair" else nnz, vmax=2 if variant == "stair" else 4, modes=tuple(modes),
                            policies=tuple(dict(p) for p in policies)))
        if kernel == "attn_text_kernel":
            cs.out_trail = 56
        arm = expected_arm(Case(cs.name, kernel, heads, d, mode_desc(cs, modes[0])), policies[0])
        cs.meta["arm"] = arm
        cs.meta["spike_rows"], cs.meta["spike_keys"] = _spike_sets(desc, arm) if variant == "spike" else ([], [])
        out.append(cs)


def _cases():
    out = []
    both, sc = ("q_log2", "scale"), ("scale",)
    std, stair = ("plain", "shift", "spike"), ("plain", "shift", "spike", "stair")
    g = "attn_kernel"
    # ---- attn_kernel: every instantiated d; NW 4, ring, masked tail, block order "head"
    for d in (8, 16, 32, 40, 64, 80, 128, 160):      # (d >= 128: six batches, or the staircase's two entries per row leave channels with < 8 rows)
        _add(out, f"general-d{d}-110x240", g, 2, d, dict(batches=3 if d < 128 else 6, lq=110, lk=240), stair + (("high",) if d in (40, 64) else ()), both)
    # NW 1 (Lq <= 32), single buffer, with and without masked keys; block order "qtile"
    _add(out, "general-nw1-d64-17x64", g, 2, 64, dict(batches=10, lq=17, lk=64), std, both)
    _add(out, "general-nw1-d40-32x40", g, 2, 40, dict(batches=6, lq=32, lk=40), std, both)
    _add(out, "general-nw1-d160-20x33", g, 1, 160, dict(batches=16, lq=20, lk=33), std, both)
    # ring with Lk % 64 == 0, block order "qtile" (Lk <= 128, no leading segment)
    _add(out, "general-d40-70x128", g, 2, 40, dict(batches=3, lq=70, lk=128), std, both)
    _add(out, "general-d32-70x128", g, 2, 32, dict(batches=3, lq=70, lk=128), std, both)
    # NW 8 (d <= 80, Lq >= 1024) where the spatial kernel refuses: Lk < 192, policy attn_spatial 0 / 2
    _add(out, "general-nw8-d40-1030x176", g, 2, 40, dict(batches=1, lq=1030, lk=176), stair, both)
    _add(out, "general-nw8-d80-1024x190", g, 2, 80, dict(batches=1, lq=1024, lk=190), stair, both)
    _add(out, "general-nw8-d40-1024x192-spatial0", g, 2, 40, dict(batches=1, lq=1024, lk=192), stair, both, policies=({"attn_spatial": 0},))
    _add(out, "general-nw8-d80-1030x240-spatial2", g, 2, 80, dict(batches=1, lq=1030, lk=240), stair, both, policies=({"attn_spatial": 2},))
    # causal, CLIP's form
    for L in (77, 130):
        _add(out, f"general-causal-d64-{L}", g, 2, 64, dict(batches=3, lq=L, lk=L, causal=True), stair, both)
    # two segments, seg1_len not a multiple of 64 (the anchor frame's keys appended as kv batch frames + clip)
    for d in (40, 80):
        _add(out, f"general-seg50-d{d}", g, 2, d,
             dict(batches=4, lq=50, lk=100, kv_outer_rows=50, seg1_len=50, seg1_div=2, seg1_mul=1, seg1_add=4), std, both)
    # the short and the text kernel's layouts on the general kernel
    _add(out, "general-temporal-9x21-short0", g, 8, 40, _temporal(9, 21, 12), std, sc, policies=({"attn_short": 0},))
    _add(out, "general-text-lk77-text0", g, 8, 40, dict(batches=2, lq=1030, lk=77, kv_div=2, kv_outer_rows=82), std, sc,
         policies=({"attn_text": 0},))
    # ---- attn_spatial_kernel
    s = "attn_spatial_kernel"
    p40 = ({}, {"attn_opt": 0}, {"attn_pv16": 0}, {"attn_pv16": 0, "attn_opt": 0})
    p80 = ({}, {"attn_opt": 0})
    _add(out, "spatial-d40-1024x192", s, 2, 40, dict(batches=1, lq=1024, lk=192), stair + ("high",), both, p40)
    _add(out, "spatial-d40-1030x677", s, 2, 40, dict(batches=1, lq=1030, lk=677), stair, both, p40)
    _add(out, "spatial-d80-1030x640", s, 2, 80, dict(batches=1, lq=1030, lk=640), stair, both, p80)
    _add(out, "spatial-d80-1024x677", s, 1, 80, dict(batches=2, lq=1024, lk=677), stair, both, p80)
    seg = dict(batches=2, lq=1024, lk=320, kv_outer_rows=192, seg1_len=128, seg1_div=2, seg1_mul=1, seg1_add=2)
    _add(out, "spatial-seg128-d40", s, 1, 40, seg, stair, both, p40)
    _add(out, "spatial-seg128-d80", s, 1, 80, seg, stair, both, p80)
    # ---- attn_short_kernel: whole 320-channel groups, temporal row strides
    for d, heads in ((40, 8), (80, 4), (160, 2)):
        for tl, tg in ((1, 1), (3, 17), (17, 17), (9, 21)):
            _add(out, f"short-d{d}-{tl}x{tg}", "attn_short_kernel", heads, d, _temporal(tl, tg, 64 if tl <= 3 else 24), std, sc,
                 nnz=12 if tl == 1 else 4)
    # ---- attn_text_kernel: Lq * kv_div just >= 2048 and ragged
    for d, heads in ((40, 8), (80, 4)):
        for lk in (64, 77, 96):
            _add(out, f"text-d{d}-lk{lk}", "attn_text_kernel", heads, d, dict(batches=2, lq=1030, lk=lk, kv_div=2, kv_outer_rows=lk + 5), std, sc)
    for i, cs in enumerate(out):
        cs.seed = 1000 + 7 * i
    return out


CASES = _cases()
BY_NAME = {cs.name: cs for cs in CASES}
assert len(BY_NAME) == len(CASES)
