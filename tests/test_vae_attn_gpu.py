"""The first stage's mid-block attention (ccedit_amd/vae.py: AttnBlock.run, bf16; ccedit_amd/vae_f32.py: attn_block, fp32 under both
values of library policy `f32_split`) against the float64 reference of tests/_vae_attn_ref.py at ragged frame sizes: L % 4 != 0, L < 16,
L straddling the 128 / 256 tile edges, L across the fp32 dispatch threshold (M >= 4096 and N > 128: the pipelined kernel), L > 8192 (the
re-reading softmax), more than one frame (the last frame's operand padding differs from the others').  Every frame is judged on its own:
max-abs error and relative RMS of the branch (out - x) within 8 x (fp32 arms) / 2 x (bf16 arm) the same figures of the CPU emulation
of that arm, the whole block below F32_VAE_TOL / VAE_TOL.  tests/test_vae_attn_ref.py shows on the CPU that these bounds pass a correct
evaluation in another summation order and catch every planted defect.  Then the three GEMM roles of the fp32 arms directly (an
activation matrix as the "weight", ldc > N, pad columns and rows that must not be read or written), per element against the fp32
accumulation bound, and the whole first stage at two ragged frame sizes against the CPU oracle.

Measured on the first GPU run on an MI355X (figure / bound; 1.0 is the bound; run with -s for every case and frame):
  block, bf16 arm           max-abs 0.500 ... 0.566, branch RMS 0.499 ... 0.503 on all 15 frames of the 7 cases (the kernels land on the
                            emulation's bf16 values almost everywhere: 0.5 is the emulation itself under the 2 x margin); whole block
                            0.056 ... 0.076 of VAE_TOL
  block, six bf16 products  max-abs 0.085 ... 0.325, branch RMS 0.082 ... 0.184, whole block <= 0.009 of F32_VAE_TOL;
                            17 x 241 (pipelined kernel) 0.253 / 0.274 / 0.009, 82 x 100 (re-reading softmax) 0.346 / 0.378 / 0.011
  block, fp32 MFMA          max-abs 0.106 ... 0.346, branch RMS 0.080 ... 0.255, whole block <= 0.011;
                            17 x 241 0.268 / 0.388 / 0.013, 82 x 100 0.641 / 0.592 / 0.018
  GEMM roles, max |err| / bound over the elements (six bf16 products | fp32 MFMA):
      L = 6, c = 128        q k^T 0.0070 | 0.0073   V^T 0.0165 | 0.0241   p v 0.1467 | 0.1929
      L = 35, c = 128       q k^T 0.0174 | 0.0200   V^T 0.0276 | 0.0206   p v 0.0806 | 0.1113
      L = 117, c = 128      q k^T 0.0206 | 0.0408   V^T 0.0231 | 0.0249   p v 0.0299 | 0.0391
      L = 132, c = 128      q k^T 0.0206 | 0.0243   V^T 0.0197 | 0.0266   p v 0.0334 | 0.0425
      L = 132, c = 512      q k^T 0.0061 | 0.0060   V^T 0.0079 | 0.0083   p v 0.0478 | 0.0418
      L = 4097, c = 512     q k^T 0.0106 | 0.0150   V^T 0.0095 | 0.0112   p v 0.0024 | 0.0042
  whole first stage against the CPU oracle, relative RMS (decode, encode):
      40 x 56 px            bf16 1.46e-2, 6.12e-3   six bf16 products 1.76e-6, 8.84e-7   fp32 MFMA 2.25e-6, 8.50e-7
      136 x 184 px          bf16 1.34e-2, 6.13e-3   six bf16 products 1.72e-6, 7.70e-7   fp32 MFMA 2.12e-6, 8.33e-7
No kernel or host code needed a change: every case passed as the code stood.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _vae_attn_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu

ARMS = {"bf16": None, "six-bf16-products": 1, "mfma-f32": 0}
SENTINEL = 7.0


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


@pytest.fixture(params=list(ARMS), ids=list(ARMS))
def arm(request):
    """bf16: AttnBlock.run.  The other two: vae_f32.attn_block under library policy `f32_split` = 1 (six exact bf16 x bf16 products per
    fp32 product) and 0 (v_mfma_f32_32x32x2_f32), restored afterwards — the fixture of test_vae_f32_gpu.py."""
    _dev()
    from ccedit_amd import hip
    split = ARMS[request.param]
    if split is not None:
        assert hip.lib().ccedit_policy_set(b"f32_split", split) == 0
    yield request.param
    hip.lib().ccedit_policy_set(b"f32_split", 1)


@pytest.fixture(params=[1, 0], ids=["six-bf16-products", "mfma-f32"])
def split(request):
    _dev()
    from ccedit_amd import hip
    assert hip.lib().ccedit_policy_set(b"f32_split", request.param) == 0
    yield request.param
    hip.lib().ccedit_policy_set(b"f32_split", 1)


_blocks = {}


def _block(c):
    """AttnBlock(c) alone, filled by the name-keyed rule under the decoder's prefix (the parameters of P.case) and packed."""
    if c not in _blocks:
        from ccedit_amd.layers import pack_tree
        from ccedit_amd.utils.synth import fill_module_
        from ccedit_amd.vae import AttnBlock
        blk = AttnBlock(c)
        fill_module_(blk, prefix=P.PREFIX)
        pack_tree(blk, torch.device("cuda:0"))
        _blocks[c] = blk
    return _blocks[c]


def _run_block(arm, shape):
    dev = _dev()
    from ccedit_amd import vae_f32
    cs = P.case(*shape)
    blk = _block(cs.c)
    assert torch.equal(blk.q.weight.reshape(cs.c, cs.c), cs.w_q) and torch.equal(blk.v.bias, cs.b_v) and torch.equal(blk.norm.weight, cs.gamma)
    x = cs.x.reshape(cs.n, cs.h, cs.w, cs.c).to(device=dev, dtype=torch.bfloat16 if arm == "bf16" else torch.float32).contiguous()
    keep = x.clone()
    run = blk.run if arm == "bf16" else (lambda t: vae_f32.attn_block(blk, t))
    out = run(x)
    assert out.shape == (cs.n, cs.h, cs.w, cs.c) and out.dtype == x.dtype
    again = run(x)
    assert torch.equal(out, again), "a second call gives other bits"
    assert torch.equal(x, keep), "the block wrote its input"
    assert torch.isfinite(out).all()
    got = out.reshape(cs.n, cs.L, cs.c).float().cpu()
    if cs.rows is not None:
        got = got[:, cs.rows]
    ratios = P.judge(got, cs, arm)
    for f, r in enumerate(ratios):
        print(f"attn block {P.case_id(shape)} {arm} frame {f}: max-abs {r[0]:.3f}, branch rms {r[1]:.3f}, block rms {r[2]:.3f} of their bounds")
    assert P.passes(ratios), ratios


@pytest.mark.parametrize("shape", P.BLOCK_CASES, ids=P.case_id)
def test_attn_block_vs_float64(arm, shape):
    _run_block(arm, shape)


@pytest.mark.parametrize("shape", P.LONG_CASES, ids=P.case_id)
def test_attn_block_long_frames_vs_float64(split, shape):
    """fp32 arms only (the bf16 arm refuses more than 8192 padded score columns): 17 x 241 reaches the pipelined GEMM kernel with ragged M
    and N, 82 x 100 the re-reading softmax kernel.  The float64 reference covers 256 query rows: the first 64, the last 64, 128 seeded."""
    _run_block("six-bf16-products" if split else "mfma-f32", shape)


# ------------------------------------------------------------------------------------------ the GEMM roles of the fp32 arms
def _label():
    from ccedit_amd import hip
    return (hip.lib().ccedit_last_kernel() or b"").decode()


def _check_label(split, m, n):
    name = _label()
    if not split:
        assert name.startswith("f32_gemm_kernel"), name
    elif m >= 4096 and n > 128:
        assert name.startswith("f32p_gemm_kernel"), name
    else:
        assert name.startswith("f32s_gemm_kernel 128ch x 256pix"), name


def _inside(got, ref, bnd, what):
    err = (got.detach().double().cpu() - ref).abs()
    worst = (err / bnd).max().item()
    print(f"   {what}: max |err| / bound {worst:.4f}")
    assert torch.isfinite(got).all() and worst <= 1.0, what


_role_refs = {}


@pytest.mark.parametrize("L,c", [(6, 128), (35, 128), (117, 128), (132, 128), (132, 512), (4097, 512)], ids=lambda v: str(v))
def test_gemm_roles_per_element(split, L, c):
    """q k^T, V^T and p v as attn_block issues them, each element within (K + 8) 2^-24 sum_k |a_k w_k| + half an ulp of the result."""
    dev = _dev()
    from ccedit_amd import vae_f32 as V
    l4, l16, c16 = P.ceil_to(L, 4), P.ceil_to(L, 16), P.ceil_to(c, 16)
    q, act, wv, bv = P.role_inputs(L, c)
    qd, actd, wvd, bvd = q.to(dev), act.to(dev), wv.to(dev), bv.to(dev)
    q64, k64, wv64 = q.double(), act[:L].double(), wv.double()
    print(f"GEMM roles L={L} c={c} f32_split={split}")
    # q k^T: W is a row slice of a larger activation tensor (the rows after it hold 1e30), out has row stride ceil4(L) and zero pad columns
    s = torch.zeros((L, l4), dtype=torch.float32, device=dev)
    V.gemm_f32(qd, V.PackedF32(actd[:L], None, L, c, c16, 1), out=s)
    _check_label(split, L, L)
    if (L, c) not in _role_refs:                     # shared by the two arms: the operands are the same
        r1, r2 = q64 @ k64.t(), wv64 @ k64.t()
        _role_refs[(L, c)] = (r1, P.gemm_bound(q64, k64, r1, c), r2, P.gemm_bound(wv64, k64, r2, c))
    ref_qk, bnd_qk, ref_vt, bnd_vt = _role_refs[(L, c)]
    _inside(s[:, :L], ref_qk, bnd_qk, "q k^T")
    assert (s[:, L:] == 0).all(), "q k^T wrote the pad columns of the score matrix"
    s_host = s.double().cpu()
    scale = float(c) ** -0.5
    V.softmax_rows_f32_(s, L, scale)
    assert (s[:, L:] == 0).all(), "the softmax wrote the pad columns of the score matrix"
    p64 = s.double().cpu()
    assert _rel(p64[:, :L], torch.softmax(s_host[:, :L] * scale, dim=-1)) < 5e-6           # (test_softmax_rows_f32's tolerance)
    # V^T: A is the c x c weight, W the frame's activations; out [c][ceil16(L)] keeps its sentinel from column L on
    vt = torch.full((c, l16), SENTINEL, dtype=torch.float32, device=dev)
    V.gemm_f32(wvd, V.PackedF32(actd[:L], None, L, c, c16, 1), out=vt)
    _check_label(split, c, L)
    _inside(vt[:, :L], ref_vt, bnd_vt, "V^T")
    assert (vt[:, L:] == SENTINEL).all(), "V^T wrote columns beyond L"
    # p v: Cin = ceil4(L), Cpad = ceil16(L), the v bias added after the product; A is the softmax output above
    vt0 = torch.zeros((c, l16), dtype=torch.float32, device=dev)
    vt0[:, :L] = vt[:, :L]
    o = torch.full((L, c), SENTINEL, dtype=torch.float32, device=dev)
    V.gemm_f32(s, V.PackedF32(vt0, bvd, c, l4, l16, 1), out=o)
    _check_label(split, L, c)
    v64 = vt0.double().cpu()[:, :L]
    ref = p64[:, :L] @ v64.t() + bv.double()
    _inside(o, ref, P.gemm_bound(p64[:, :L], v64, ref, L), "p v")


# ------------------------------------------------------------------------------------------ the whole first stage at ragged frames
_stage = {}


def _first_stage():
    """build_vae(ch=32) packed, and the CPU oracle's decode / encode of two frames at each size on the same state dict (computed once)."""
    if not _stage:
        from ccedit_amd.sgm_compat import build_vae
        from ccedit_amd.utils.synth import fill_module_
        from oracle import ccedit_oracle as O
        vae = build_vae("cpu", ch=32)
        fill_module_(vae, prefix="first_stage_model.")
        sd = {"first_stage_model." + k: v.clone() for k, v in vae.state_dict().items()}
        vae.pack("cuda")
        cfg = O.VAEConfig(ch=32)
        g = torch.Generator().manual_seed(2024)
        for lh, lw in ((5, 7), (17, 23)):
            z = torch.randn(1, 4, 2, lh, lw, generator=g)
            x = torch.rand(1, 3, 2, 8 * lh, 8 * lw, generator=g) * 2 - 1
            noise = torch.randn(2, 4, lh, lw, generator=g)
            _stage[(lh, lw)] = dict(z=z, x=x, noise=noise, dec=O.vae_decode(sd, "first_stage_model", cfg, z, 1.0),
                                    enc=O.vae_encode(sd, "first_stage_model", cfg, x, noise, 1.0))
        _stage["vae"] = vae
    return _stage


@pytest.mark.parametrize("lh,lw", [(5, 7), (17, 23)], ids=["40x56px", "136x184px"])
def test_first_stage_at_ragged_frames_vs_oracle(arm, lh, lw):
    _dev()
    st = _first_stage()
    vae, d = st["vae"], st[(lh, lw)]
    vae.precision = "bf16" if arm == "bf16" else "fp32"
    tol = P.VAE_TOL if arm == "bf16" else P.F32_VAE_TOL
    dec = vae.decode(d["z"].cuda())
    assert dec.shape == (1, 3, 2, 8 * lh, 8 * lw) and dec.dtype == torch.float32
    enc = vae.encode(d["x"].cuda(), noise=d["noise"])
    assert enc.shape == (1, 4, 2, lh, lw)
    rd, re = _rel(dec, d["dec"]), _rel(enc, d["enc"])
    print(f"first stage {8 * lh}x{8 * lw} px {arm}: decode rel rms {rd:.2e}, encode rel rms {re:.2e} (tolerance {tol:.0e})")
    assert rd < tol and re < tol
