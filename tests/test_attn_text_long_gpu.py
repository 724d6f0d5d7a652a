"""attn_text_long_kernel (csrc/attntextlong.hip) on a real MI355X: text cross-attention onto the 154 / 231 / 308 keys of a long prompt
(ccedit_amd/prompt.py).  The call pattern of tests/test_ops_gpu.py::test_text_cross_attention_kernel — queries a column slice of a wider
buffer, K / V column slices of the fused [clips (Lk + 5), 2 C] projection whose gap rows are NaN — against a float64 reference under the
project's attention bound (rel 2^-6, abs 4e-3), the same launch with the arm switched off (policy attn_text = 0), reruns, a strided
output with NaN guard columns, a spiked key at both ends of the key range, and all-equal scores.

With attn_text = 0 the launch goes where it went before the arm existed, which tests/_attn_cases.expected_arm restates: attn_kernel at
154 keys and wherever Lq < 1024, attn_spatial_kernel at 231 / 308 keys with Lq >= 1024 (that kernel takes any Lq >= 1024, Lk >= 192)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attn_cases as AC  # noqa: E402

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
KEPT_LK = (154, 231, 308)            # the (d, Lk) the arm keeps: d = 80 with every one of the three key counts;
GAP = 5                              # rows between two clips' keys in the fused buffer              d = 40 lost the measurement and is out
# (d, heads, Lq, frames per clip, clips): the issue's four cases.  Its d = 40 rows are not the arm's any more (NOT_KEPT below checks where
# they go instead), so each is restated at d = 80 with the same row counts and clips — 4, 8 and 16 groups of 80 channels:
SHAPES = [(80, 4, 1100, 2, 2),       # base case
          (80, 4, 1101, 2, 1),       # ragged
          (80, 8, 700, 3, 2),        # two 320-channel groups, K / V restaged per clip
          (80, 16, 600, 4, 2)]       # 16 heads
NOT_KEPT = [(40, 8, 1100, 2, 2), (40, 8, 1101, 2, 1), (40, 16, 600, 4, 2)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF).float()     # bf16-representable fp32


def _ref64(q, k, v, heads):
    """softmax(Q K^T d^-0.5) V per head in float64: q (n, lq, c), k / v (n, lk, c)."""
    n, lq, c = q.shape
    d = c // heads
    qh = q.double().reshape(n, lq, heads, d).transpose(1, 2)
    kh = k.double().reshape(n, -1, heads, d).transpose(1, 2)
    vh = v.double().reshape(n, -1, heads, d).transpose(1, 2)
    p = torch.softmax(qh @ kh.transpose(-1, -2) * d ** -0.5, dim=-1)
    return (p @ vh).transpose(1, 2).reshape(n, lq, c)


def _close(got, ref, what):
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), what
    err = (got - ref).abs().max().item()
    lim = 2.0 ** -6 * ref.abs().max().item() + 4e-3
    print(f"{what}: max err {err:.4g} (limit {lim:.4g})")
    assert err <= lim, f"{what}: max err {err:.4g} > {lim:.4g}"


class Launch:
    """One text cross-attention launch in the network's layout."""

    def __init__(self, d, heads, lq, fpc, clips, lk, seed=0, q=None, k=None, v=None):
        self.d, self.heads, self.lq, self.fpc, self.clips, self.lk = d, heads, lq, fpc, clips, lk
        c = self.c = heads * d
        n = self.n = clips * fpc
        self.q = _rnd(n, lq, c, seed=seed + 2) if q is None else q                       # (n, lq, c)
        self.k = _rnd(clips, lk, c, seed=seed + 3) if k is None else k                   # (clips, lk, c)
        self.v = _rnd(clips, lk, c, seed=seed + 4) if v is None else v
        qbuf = _rnd(n * lq, c + 64, seed=seed + 5)                                       # q = columns [32, 32 + c) of a wider buffer
        qbuf[:, 32:32 + c] = self.q.reshape(n * lq, c)
        kv = torch.full((clips, lk + GAP, 2 * c), float("nan"))                          # the gap rows are never read
        kv[:, :lk, :c], kv[:, :lk, c:] = self.k, self.v
        self.qd, self.kvd = qbuf.to(BF).cuda(), kv.reshape(clips * (lk + GAP), 2 * c).to(BF).cuda()

    def run(self, out=None):
        from ccedit_amd import hip, ops
        c = self.c
        o = ops.attention(self.qd[:, 32:32 + c], self.kvd[:, :c], self.kvd[:, c:], self.heads, self.d, batches=self.n, lq=self.lq, lk=self.lk,
                          kv_div=self.fpc, kv_outer_rows=self.lk + GAP, out=out)
        return o, hip.lib().ccedit_last_kernel().decode()

    def run_general(self):
        from ccedit_amd import hip
        lib = hip.lib()
        assert lib.ccedit_policy_set(b"attn_text", 0) == 0
        try:
            return self.run()
        finally:
            lib.ccedit_policy_set(b"attn_text", 1)

    def ref(self):
        kk = self.k.repeat_interleave(self.fpc, 0)
        vv = self.v.repeat_interleave(self.fpc, 0)
        return _ref64(self.q, kk, vv, self.heads)


@pytest.mark.parametrize("lk", KEPT_LK)
@pytest.mark.parametrize("d,heads,lq,fpc,clips", SHAPES)
def test_long_text_arm_against_float64_and_the_general_kernel(d, heads, lq, fpc, clips, lk):
    _dev()
    L = Launch(d, heads, lq, fpc, clips, lk, seed=lk + d)
    o, name = L.run()
    assert name == f"attn_text_long_kernel d={d}", name
    ref = L.ref()
    _close(o.reshape(L.n, lq, L.c), ref, f"long text arm d={d} heads={heads} {lq}x{lk}")
    for _ in range(2):
        assert torch.equal(L.run()[0], o)
    g, gname = L.run_general()
    case = AC.Case("long-text", "attn_kernel", heads, d, dict(batches=L.n, lq=lq, lk=lk, kv_div=fpc, kv_outer_rows=lk + GAP))
    before = AC.expected_kernel(case, {"attn_text": 0})
    assert before == ("attn_spatial_kernel" if lk >= 192 and lq >= 1024 else "attn_kernel")
    assert AC.expected_kernel(case) == before, "the restated dispatch of the existing arms moved"
    assert gname == f"{before} d={d}", gname
    _close(g.reshape(L.n, lq, L.c), ref, f"{before} d={d} heads={heads} {lq}x{lk}")
    assert L.run()[1] == name                                                            # the switch is back on


@pytest.mark.parametrize("lk", KEPT_LK)
@pytest.mark.parametrize("d,heads,lq,fpc,clips", SHAPES)
def test_long_text_arm_writes_a_strided_output_and_nothing_beside_it(d, heads, lq, fpc, clips, lk):
    """The output as columns [8, 8 + C) of a wider buffer whose other columns are NaN (the `text_strided_out` cases of _attn_cases.py)."""
    _dev()
    L = Launch(d, heads, lq, fpc, clips, lk, seed=2 * lk + d)
    lead, trail = 8, 56
    buf = torch.full((L.n * lq, lead + L.c + trail), float("nan"), dtype=BF, device="cuda")
    o, name = L.run(out=buf[:, lead:lead + L.c])
    assert name == f"attn_text_long_kernel d={d}", name
    assert bool(torch.isnan(buf[:, :lead]).all()) and bool(torch.isnan(buf[:, lead + L.c:]).all())
    _close(buf[:, lead:lead + L.c].reshape(L.n, lq, L.c), L.ref(), f"strided out d={d} {lq}x{lk}")
    assert torch.equal(buf[:, lead:lead + L.c], L.run()[0])


@pytest.mark.parametrize("lk", KEPT_LK)
@pytest.mark.parametrize("key", ["last", "first"])
@pytest.mark.parametrize("d,heads,lq,fpc,clips", SHAPES)
def test_long_text_arm_with_a_spiked_key(d, heads, lq, fpc, clips, lk, key):
    """Key Lk - 1 (in the last, partly masked key tile) or key 0 carries 4 x a query row: for that row the spike owns the softmax (its
    score is 4 |q|^2 d^-0.5, tens above every other), for the other rows it is one key among many — the maximum and the masked tail."""
    _dev()
    c = heads * d
    q = _rnd(clips * fpc, lq, c, seed=lk + 11)
    k = _rnd(clips, lk, c, seed=lk + 12)
    at = lk - 1 if key == "last" else 0
    rows = (5, lq - 1)
    for ci in range(clips):
        k[ci, at] = (4.0 * q[ci * fpc, rows[ci % 2]]).to(BF).float()
    L = Launch(d, heads, lq, fpc, clips, lk, seed=lk, q=q, k=k)
    o, name = L.run()
    assert name == f"attn_text_long_kernel d={d}", name
    ref = L.ref()
    _close(o.reshape(L.n, lq, c), ref, f"spike at key {at} d={d} {lq}x{lk}")
    for ci in range(clips):                      # the spiked row is (nearly) V of the spiked key: the spike reached the maximum
        row = o.reshape(L.n, lq, c)[ci * fpc, rows[ci % 2]].float().cpu()
        assert (row - L.v[ci, at]).abs().max().item() <= 2.0 ** -6 * L.v[ci, at].abs().max().item() + 4e-3


@pytest.mark.parametrize("lk", KEPT_LK)
@pytest.mark.parametrize("d,heads,lq,fpc,clips", SHAPES)
def test_long_text_arm_with_equal_scores_gives_the_mean_of_v(d, heads, lq, fpc, clips, lk):
    _dev()
    c = heads * d
    L = Launch(d, heads, lq, fpc, clips, lk, seed=lk + 3, k=torch.zeros(clips, lk, c))
    o, name = L.run()
    assert name == f"attn_text_long_kernel d={d}", name
    mean = L.v.double().mean(dim=1).repeat_interleave(fpc, 0)[:, None].expand(-1, lq, -1)          # a padded key would pull it down
    _close(o.reshape(L.n, lq, c), mean, f"equal scores d={d} {lq}x{lk}")


@pytest.mark.parametrize("lk", KEPT_LK)
@pytest.mark.parametrize("d,heads,lq,fpc,clips", NOT_KEPT)
def test_d40_stays_where_it_was(d, heads, lq, fpc, clips, lk):
    """d = 40 was measured slower on the arm than on the existing kernels: it is outside the arm's applicability and goes where
    tests/_attn_cases.expected_arm sends it, switch on or off, with the float64 result."""
    _dev()
    L = Launch(d, heads, lq, fpc, clips, lk, seed=lk + 9)
    case = AC.Case("long-text-d40", "attn_kernel", heads, d, dict(batches=L.n, lq=lq, lk=lk, kv_div=fpc, kv_outer_rows=lk + GAP))
    o, name = L.run()
    assert name == f"{AC.expected_kernel(case)} d={d}", name
    assert L.run_general()[1] == name
    _close(o.reshape(L.n, lq, L.c), L.ref(), f"d=40 {lq}x{lk} on {name}")
