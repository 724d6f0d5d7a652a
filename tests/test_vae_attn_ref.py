"""CPU evidence for tests/test_vae_attn_gpu.py, in the manner of test_epilogue_ref.py: the float64 reference of tests/_vae_attn_ref.py
agrees with an independent formulation, a correct evaluation of the block in another summation order meets the GPU test's bounds on
every small case in both arms, and every planted defect misses them on at least one of those cases in each arm.  Also the up-front
refusal of frames the bf16 first stage cannot evaluate.  Run with -s to see the table (defect, shape, arm, figure / bound)."""
import os
import re
import sys
import types

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _vae_attn_ref as P  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_tolerances_are_the_projects():
    for fname, name, value in (("test_vae_f32_gpu.py", "F32_VAE_TOL", P.F32_VAE_TOL), ("test_network_gpu.py", "VAE_TOL", P.VAE_TOL)):
        with open(os.path.join(ROOT, "tests", fname)) as f:
            m = re.search(r"^%s = (\S+)" % name, f.read(), re.M)
        assert m and float(m.group(1)) == value, (fname, name)


def test_reference_against_an_independent_formulation():
    """The per-frame float64 reference equals the oracle's formulation of the block (convolutions and scaled_dot_product_attention on
    NCHW tensors, all frames at once) in float64, and differs from it once a frame's keys come from its neighbour."""
    for shape in ((3, 2, 2, 128), (5, 7, 3, 512)):
        cs = P.case(*shape)
        x = cs.x.double().reshape(cs.n, cs.h, cs.w, cs.c).permute(0, 3, 1, 2)
        y = F.group_norm(x, 32, cs.gamma.double(), cs.beta.double(), 1e-6)
        q, k, v = (F.conv2d(y, getattr(cs, "w_" + nm).double()[:, :, None, None], getattr(cs, "b_" + nm).double()).flatten(2).transpose(1, 2)
                   for nm in ("q", "k", "v"))
        a = F.scaled_dot_product_attention(q[:, None], k[:, None], v[:, None])[:, 0]
        br = F.conv2d(a.transpose(1, 2).reshape(cs.n, cs.c, cs.h, cs.w), cs.w_proj_out.double()[:, :, None, None], cs.b_proj_out.double())
        br = br.permute(0, 2, 3, 1).reshape(cs.n, cs.L, cs.c)
        assert (br - cs.ref).abs().max().item() <= 1e-12
        rolled = F.scaled_dot_product_attention(q[:, None], k.roll(1, 0)[:, None], v[:, None])[:, 0]
        assert (rolled - a).abs().max().item() > 1e-2, "the frames of the case do not differ enough to tell their keys apart"


def test_inputs_are_what_the_issue_asks():
    cs = P.case(5, 7, 3, 128)
    assert torch.equal(cs.x, P.bf16r(cs.x)) and cs.rows is None
    m, s = cs.x.mean(dim=(1, 2)), cs.x.std(dim=(1, 2))
    assert (m[0] - m[1]).abs() > 1 and (m[1] - m[2]).abs() > 1 and s.max() / s.min() > 4           # frames differ in mean and scale
    for nm in ("q", "k", "v", "proj_out"):
        assert getattr(cs, "b_" + nm).abs().max() > 0 and 0.7 < getattr(cs, "w_" + nm).std() * cs.c ** 0.5 < 1.3
    rows = P.long_rows(8200, 8200)
    assert rows.numel() == 256 and rows.unique().numel() == 256 and rows[:64].tolist() == list(range(64)) and rows[-64:].tolist() == list(range(8136, 8200))
    assert [c[0] * c[1] for c in P.BLOCK_CASES + P.LONG_CASES] == [6, 35, 35, 117, 132, 391, 1551, 4097, 8200]


@pytest.mark.parametrize("shape", P.BLOCK_CASES, ids=P.case_id)
@pytest.mark.parametrize("arm", ["fp32", "bf16"])
def test_correct_evaluation_in_another_order_passes(arm, shape):
    cs = P.case(*shape)
    ratios = P.judge(P.emulate(cs, arm, order="tiles"), cs, arm)
    for f, r in enumerate(ratios):
        print(f"clean (K tiles of 16, exp2) {P.case_id(shape)} {arm} frame {f}: max-abs {r[0]:.3f}, branch rms {r[1]:.3f}, block rms {r[2]:.3f} of their bounds")
    assert P.passes(ratios)


@pytest.mark.parametrize("arm", ["fp32", "bf16"])
@pytest.mark.parametrize("name,defect", P.DEFECTS, ids=[d[1] for d in P.DEFECTS])
def test_planted_defect_misses_the_bounds(name, defect, arm):
    """Each defect, in each arm, leaves the bounds on at least one small shape (a defect of the pad columns cannot show where L % 4 = 0,
    one of a frame's neighbour not in a single frame: the table says where each shows)."""
    caught = []
    for shape in P.DEFECT_CASES:
        cs = P.case(*shape)
        ratios = P.judge(P.emulate(cs, arm, defect=defect), cs, arm)
        worst = max(max(r[:2]) for r in ratios)
        miss = not P.passes(ratios)
        caught.append(miss)
        print(f"{name} | {P.case_id(shape)} | {arm} | worst figure / bound {worst:.3g} | {'MISSES' if miss else 'inside'} "
              f"(frames outside: {[f for f, r in enumerate(ratios) if max(r) > 1.0]})")
    assert any(caught), name


def test_gemm_role_bound_discriminates():
    """The per-element bound of the GEMM roles: torch's fp32 product of a role's operands is inside, a result whose last column was
    computed from the row after the slice (or from the last row but one) is outside."""
    L, c = 35, 128
    q, act, _, _ = P.role_inputs(L, c)
    k = act[:L]
    ref = q.double() @ k.double().t()
    bnd = P.gemm_bound(q.double(), k.double(), ref, c)
    got = (q @ k.t()).double()
    assert ((got - ref).abs() <= bnd).all()
    for wrong in (act[L], k[L - 2]):
        bad = got.clone()
        bad[:, L - 1] = (q @ wrong).double()
        assert ((bad - ref).abs() > bnd).any()
    assert P.ulp32(torch.tensor([1.0, 1.5, 2.0, 0.0, -0.75], dtype=torch.float64)).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 0.0, 2.0 ** -24]


# ------------------------------------------------------------------------------------------ the bf16 first stage's frame limit
def test_bf16_first_stage_refuses_long_frames_before_any_launch():
    from ccedit_amd import vae as V
    from ccedit_amd.sgm_compat import build_vae
    V.check_bf16_frame(64, 128)                     # 8192 latent pixels: the most the bf16 softmax takes
    V.check_bf16_frame(96, 85)
    with pytest.raises(ValueError, match=r"656x800 px has 8200 latent pixels.*8192.*vae_fp32=1.*disable_first_stage_autocast"):
        V.check_bf16_frame(82, 100)
    with pytest.raises(ValueError):
        V.check_bf16_frame(8193, 1)
    vae = build_vae("cpu", ch=32)
    vae._packed = True                              # (nothing is packed: the refusal comes before the first launch, also without a GPU)
    vae.precision = "bf16"
    with pytest.raises(ValueError, match="8200 latent pixels"):
        vae.decode(torch.zeros(1, 4, 2, 82, 100))
    with pytest.raises(ValueError, match="8200 latent pixels"):
        vae.decode(torch.zeros(2, 4, 100, 82))
    with pytest.raises(ValueError, match="8200 latent pixels"):
        vae.encode(torch.zeros(1, 3, 656, 800))
    with pytest.raises(ValueError, match="multiple of 8"):
        vae.encode(torch.zeros(1, 3, 652, 800))


def test_entry_point_refuses_long_frames_by_precision(tmp_path, monkeypatch):
    from ccedit_amd import policy
    from scripts.sampling import sampling_tv2v as S
    cfgs = {}
    for flag in (True, False, None):
        p = tmp_path / f"cfg_{flag}.yaml"
        p.write_text("model:\n  target: x\n  params:\n    scale_factor: 0.18215\n" + ("" if flag is None else f"    disable_first_stage_autocast: {flag}\n"))
        cfgs[flag] = str(p)
    args = lambda cfg, h=656, w=800: types.SimpleNamespace(config_path=cfg, H=h, W=w)
    real = policy.get

    def with_policy(v):
        monkeypatch.setattr(policy, "get", lambda name: v if name == "vae_fp32" else real(name))

    with_policy(2)                                  # the default: the yaml's flag decides
    assert [S.first_stage_precision(args(cfgs[f])) for f in (True, False, None)] == ["fp32", "bf16", "bf16"]
    S.check_first_stage(args(cfgs[True]))
    for f in (False, None):
        with pytest.raises(ValueError, match="8200 latent pixels"):
            S.check_first_stage(args(cfgs[f]))
        S.check_first_stage(args(cfgs[f], 512, 1024))           # 8192 latent pixels
    with_policy(1)
    assert S.first_stage_precision(args(cfgs[False])) == "fp32"
    S.check_first_stage(args(cfgs[False]))
    with_policy(0)
    assert S.first_stage_precision(args(cfgs[True])) == "bf16"
    with pytest.raises(ValueError, match="vae_fp32=1"):
        S.check_first_stage(args(cfgs[True]))
    S.check_first_stage(args(cfgs[True], 650, 800))             # not a multiple of 8: refused where the frames are read, with its own message
