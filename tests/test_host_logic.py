"""CPU tests of the host logic: config/operator API, state-dict contract, packing, sampling scalars."""
import json
import os

import numpy as np
import pytest
import torch


def test_reference_config_instantiates_with_reference_keys(golden_dir):
    """The reference's own yaml (copied structure) resolves through instantiate_from_config to this build's
    classes and yields exactly the reference's state-dict keys and shapes (golden: keys_tv2v.json)."""
    from ccedit_amd.config import Config, instantiate_from_config
    dd = "sgm.modules.diffusionmodules."
    net = dict(use_checkpoint=False, in_channels=4, out_channels=4, model_channels=320, attention_resolutions=[4, 2, 1],
               num_res_blocks=2, channel_mult=[1, 2, 4, 4], num_heads=8, use_spatial_transformer=True, transformer_depth=1,
               context_dim=768, legacy=False, disable_temporal_text_ca=True)
    cn = {k: v for k, v in net.items() if k not in ("out_channels", "disable_temporal_text_ca")}
    cn.update(hint_channels=3, control_scales=1.0)
    net["controlnet_config"] = dict(target=dd + "controlmodel.ControlNet2D", params=cn)
    cfg = Config(model=dict(target="sgm.models.diffusion.VideoDiffusionEngineTV2V", params=dict(
        use_ema=False, scale_factor=0.18215, disable_first_stage_autocast=True, log_keys=["txt"], freeze_model="spatial",
        denoiser_config=dict(target=dd + "denoiser.DiscreteDenoiser", params=dict(
            num_idx=1000, weighting_config=dict(target=dd + "denoiser_weighting.EpsWeighting"),
            scaling_config=dict(target=dd + "denoiser_scaling.EpsScaling"),
            discretization_config=dict(target=dd + "discretizer.LegacyDDPMDiscretization"))),
        network_config=dict(target=dd + "controlmodel.ControlledUNetModel3DTV2V", params=net),
        conditioner_config=dict(target="sgm.modules.GeneralConditioner", params=dict(emb_models=[
            dict(is_trainable=False, input_key="txt", ucg_rate=0.5, target="sgm.modules.encoders.modules.FrozenCLIPEmbedder"),
            dict(is_trainable=False, input_key="control_hint", target="sgm.modules.encoders.modules.DepthMidasEncoder")])),
        first_stage_config=dict(target="sgm.models.autoencoder.AutoencoderKLInferenceWrapper", params=dict(
            embed_dim=4, monitor="val/rec_loss", lossconfig=dict(target="torch.nn.Identity"),
            ddconfig=dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4, 4],
                          num_res_blocks=2, attn_resolutions=[], dropout=0.0))))))
    with torch.device("meta"):
        engine = instantiate_from_config(cfg["model"])
    mine = {k: list(v.shape) for k, v in engine.state_dict().items()}
    with open(os.path.join(golden_dir, "keys_tv2v.json")) as f:
        ref = json.load(f)
    assert set(ref) - set(mine) == set(), sorted(set(ref) - set(mine))[:5]
    extra = set(mine) - set(ref)
    clip = {k for k in extra if k.startswith("conditioner.embedders.0.transformer.text_model.")}
    assert extra - clip == {"denoiser.sigmas"}
    with open(os.path.join(golden_dir, "keys_clip_text.json")) as f:
        clip_ref = json.load(f)                  # HF CLIPTextModel keys (+ the position_ids buffer of transformers 4.19.1)
    assert clip - {"conditioner.embedders.0.transformer.text_model.embeddings.position_ids"} == set(clip_ref)
    assert all(mine[k] == clip_ref[k] for k in clip_ref)
    assert all(mine[k] == ref[k] for k in ref)
    n = sum(int(np.prod(s)) for k, s in mine.items() if k.startswith("model."))
    assert n == 1608747976            # 1608.7 M parameters
    assert engine.scale_factor == 0.18215 and hasattr(engine.model, "diffusion_model")
    assert hasattr(engine.model.diffusion_model, "controlnet") and hasattr(engine.model.diffusion_model, "input_blocks_temporal")


def test_instantiate_error_conventions():
    from ccedit_amd.config import instantiate_from_config
    with pytest.raises(KeyError):
        instantiate_from_config({"params": {}})
    assert instantiate_from_config("__is_first_stage__") is None
    assert instantiate_from_config("__is_unconditional__") is None


def test_unsupported_options_fail_loudly():
    from ccedit_amd.sgm_compat import network_params
    from ccedit_amd.network import ControlledUNetModel3DTV2V
    p = network_params(model_channels=32, num_heads=2, context_dim=32)
    p["use_scale_shift_norm"] = True
    with pytest.raises(NotImplementedError):
        with torch.device("meta"):
            ControlledUNetModel3DTV2V(**p)


def test_sigma_schedule_and_quantisation_bit_exact(golden_dir):
    from ccedit_amd.sampling import DiscreteDenoiser, LegacyDDPMDiscretization
    z = np.load(os.path.join(golden_dir, "sigmas.npz"))
    disc = LegacyDDPMDiscretization()
    for n in (5, 30, 50):
        got = disc(n, device="cpu").numpy()
        assert got.dtype == np.float32 and np.array_equal(got, z[f"sampler_{n}"])
    dd = "sgm.modules.diffusionmodules."
    den = DiscreteDenoiser(dict(target=dd + "denoiser_weighting.EpsWeighting"), dict(target=dd + "denoiser_scaling.EpsScaling"),
                           1000, dict(target=dd + "discretizer.LegacyDDPMDiscretization"))
    assert np.array_equal(den.sigmas.numpy(), z["denoiser_1000"])
    idx = den.sigma_to_idx(torch.from_numpy(z["probe_sigma"]))
    assert idx.dtype == torch.int64 and np.array_equal(idx.numpy(), z["probe_idx"])


def test_dpmpp2s_scalars_match_oracle():
    """Host-side scalar math of one sampler step == the oracle's tensor math (same fp32 op order)."""
    from ccedit_amd.sampling import DPMPP2SAncestralSampler, get_ancestral_step
    from oracle import ccedit_oracle as O
    dd = "sgm.modules.diffusionmodules."
    s = DPMPP2SAncestralSampler(num_steps=30, discretization_config=dict(target=dd + "discretizer.LegacyDDPMDiscretization"),
                                guider_config=dict(target=dd + "guiders.VanillaCFGTV2V", params=dict(scale=7.5)), device="cpu")
    sig = O.sampler_sigmas(30)
    for i in (0, 7, 28):
        a, b = sig[i:i + 1], sig[i + 1:i + 2]
        down, up = get_ancestral_step(a, b, 1.0)
        d2, u2 = O.ancestral_step_sigmas(a, b, 1.0)
        assert torch.equal(down, d2) and torch.equal(up, u2)
        h, ss, t, tn = s.get_variables(a, down)
        m = s.get_mult(h, ss, t, tn)
        assert torch.equal(m[0], (-ss).exp() / (-t).exp()) and torch.equal(m[3], (-h).expm1())
    # eta=1: sigma(s) = sqrt(sigma_i * sigma_down) lands on the next table entry -> index trace [t0,t1,t1,t2,...]
    table = O.denoiser_sigmas(1000)
    down, _ = get_ancestral_step(sig[0:1], sig[1:2], 1.0)
    h, ss, t, tn = s.get_variables(sig[0:1], down)
    assert O.sigma_to_idx(table, (-ss).exp()).item() == O.sigma_to_idx(table, sig[1:2]).item()


def test_packing_layouts():
    from ccedit_amd.packing import pack_concat, pack_weight
    w = torch.arange(2 * 3 * 9, dtype=torch.float32).reshape(2, 3, 3, 3)
    pw = pack_weight(w, torch.tensor([1.0, 2.0]))
    assert pw.w.shape == (256, 128) and pw.cin == 8 and pw.taps == 9 and pw.kpad == 128 and pw.n == 4
    # K index = tap*Cin_pad + c ; tap = ky*3+kx
    assert pw.w[1, 4 * 8 + 2].float().item() == w[1, 2, 1, 1].item()
    assert pw.w[0, 3].item() == 0 and pw.w[2].abs().sum().item() == 0
    assert pw.bias.tolist() == [1.0, 2.0, 0.0, 0.0]
    wk = torch.randn(3, 128, 3, 3)
    pk = pack_weight(wk)
    assert pk.korder == 1 and pk.kpad == 9 * 128
    # chunk-major: K index = chunk*(9*64) + tap*64 + c
    assert pk.w[2, 1 * 576 + 5 * 64 + 7].float().item() == wk[2, 64 + 7, 1, 2].to(torch.bfloat16).float().item()
    w1 = torch.randn(5, 16, 3)
    p1 = pack_weight(w1)
    assert torch.equal(p1.w[:5, 16:32].float(), w1[:, :, 1].to(torch.bfloat16).float())
    g = torch.arange(32 * 8, dtype=torch.float32).reshape(32, 8)        # GEGLU: 16 value rows then 16 gate rows
    pg = pack_weight(g, geglu=True)
    rows = pg.w[:32, 0].float() / 8
    assert rows.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 16, 17, 18, 19, 20, 21, 22, 23, 8, 9, 10, 11, 12, 13, 14, 15,
                             24, 25, 26, 27, 28, 29, 30, 31]
    assert pg.n == 32 and pg.n_out == 16
    pc = pack_concat([torch.ones(4, 8), 2 * torch.ones(4, 8), 3 * torch.ones(8, 8)])
    assert pc.n == 16 and pc.w[5, 0].item() == 2 and pc.w[15, 7].item() == 3


def test_fragment_ordered_weight_copy():
    """PackedWeight.wfrag (CcGemmDesc.Wfrag, ABI 12): the K = 320 / 640 / 960 matrices once more as the 16 x 32 blocks one
    v_mfma_f32_16x16x32_bf16 A operand holds — block (t, s) is 64 lanes x 8 elements, lane (g, c) = W[16 t + c][32 s + 8 g .. + 7] —
    so that the register-resident-weight kernels preload a fragment as one contiguous kilobyte.  Same values as `w`; only the widths
    those kernels serve carry it."""
    from ccedit_amd.packing import fold_layernorm, fragment_order, pack_concat, pack_weight
    g = torch.Generator().manual_seed(5)
    for shape in ((640, 640), (320, 320), (1920, 640), (320, 320, 3), (64, 640)):
        pw = pack_weight(torch.randn(*shape, generator=g))
        assert pw.wfrag is not None and pw.wfrag.numel() == pw.w.numel(), shape
        rows, kpad = pw.w.shape
        f = pw.wfrag.view(rows // 16, kpad // 32, 64, 8)
        for t, s_, lane in ((0, 0, 0), (1, 3, 17), (rows // 16 - 1, kpad // 32 - 1, 63), (2, 5, 40)):
            gq, c = lane >> 4, lane & 15
            assert torch.equal(f[t, s_, lane], pw.w[16 * t + c, 32 * s_ + 8 * gq: 32 * s_ + 8 * gq + 8]), (shape, t, s_, lane)
        assert torch.equal(fragment_order(pw.w), pw.wfrag)
    assert pack_concat([torch.randn(640, 640, generator=g)] * 3).wfrag is not None                   # fused q, k, v
    assert fold_layernorm([torch.randn(640, 640, generator=g)], [None], torch.ones(640), torch.zeros(640)).wfrag is not None
    for shape in ((1280, 1280), (320, 320, 3, 3), (640, 2560), (1280, 1280, 3)):                   # widths no such kernel serves
        assert pack_weight(torch.randn(*shape, generator=g)).wfrag is None, shape


def test_fp32_first_stage_packing_and_policy():
    """ccedit_amd/vae_f32.py host side (no GPU): the fp32 kernel layout — [Cout][tap][Cpad], tap = 3 ky + kx, zero columns beyond Cin,
    Cin rounded up to 4 for the activation rows — and the policy entry that selects the fp32 first stage (default 2: whatever the yaml's disable_first_stage_autocast says)."""
    from ccedit_amd import policy
    from ccedit_amd.vae_f32 import pack_f32
    w = torch.arange(5 * 6 * 9, dtype=torch.float32).reshape(5, 6, 3, 3)
    pw = pack_f32(w, torch.arange(5.0), "cpu")
    assert pw.w.shape == (5, 9 * 16) and pw.w.dtype == torch.float32 and (pw.n, pw.cin, pw.cpad, pw.taps) == (5, 8, 16, 9)
    assert pw.w[3, 7 * 16 + 4].item() == w[3, 4, 2, 1].item()          # tap 7 = (ky 2, kx 1)
    assert pw.w.view(5, 9, 16)[:, :, 6:].abs().sum().item() == 0        # pad columns
    assert pw.bias.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
    p1 = pack_f32(torch.randn(7, 512, 1, 1), None, "cpu")
    assert p1.w.shape == (7, 512) and p1.taps == 1 and p1.bias is None and p1.cin == 512
    p3 = pack_f32(torch.randn(128, 3, 3, 3), None, "cpu")             # the encoder's conv_in: RGB frames carry a fourth, zero channel
    assert (p3.cin, p3.cpad) == (4, 16)
    # default 2 since round 6: the engine follows the yaml's flag (the shipped yamls set it => the reference's fp32 first stage); a
    # precision choice, not a kernel arm: the generic-kernels policy string leaves it alone
    assert policy.TABLE["vae_fp32"][0] == 2 and "vae_fp32" not in policy.generic()
    from ccedit_amd.sgm_compat import build_vae
    assert build_vae("cpu", ch=32).precision == ("fp32" if policy.get("vae_fp32") == 1 else "bf16")
    # vae_fp32=2: the engine follows the yaml's disable_first_stage_autocast, as the reference does (diffusion.py:151-156)
    import subprocess, sys, os
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    code = ("from ccedit_amd.config import instantiate_from_config; from ccedit_amd.sgm_compat import engine_config; "
            "cfg = engine_config(vae_ch=32, model_channels=32, num_heads=1, context_dim=32); "
            "a = instantiate_from_config(cfg).first_stage_model.precision; cfg['params']['disable_first_stage_autocast'] = False; "
            "print(a, instantiate_from_config(cfg).first_stage_model.precision)")
    for pol, want in (("", "fp32 bf16"), ("vae_fp32=2", "fp32 bf16"), ("vae_fp32=1", "fp32 fp32"), ("vae_fp32=0", "bf16 bf16")):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CCEDIT_POLICY=pol, PYTHONPATH=root), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-1500:]
        assert r.stdout.strip().splitlines()[-1] == want, (pol, r.stdout)


def test_synth_weights_are_name_keyed_and_stable():
    from ccedit_amd.utils.synth import synth_tensor
    a = synth_tensor("model.diffusion_model.out.2.weight", (4, 320, 3, 3))
    b = synth_tensor("model.diffusion_model.out.2.weight", (4, 320, 3, 3))
    c = synth_tensor("model.diffusion_model.out.2.bias", (4,))
    assert torch.equal(a, b) and a.std().item() == pytest.approx((1 / 2880) ** 0.5, rel=0.1) and c.abs().max() < 0.2
    # pinned values: the golden vectors depend on this rule never changing
    assert a.flatten()[:3].tolist() == pytest.approx([0.005066306330263615, -0.01827041432261467, -0.0302837323397398], abs=1e-7)


# ------------------------------------------------------------------------------------------------------
# the reference's shipped inference yamls
# ------------------------------------------------------------------------------------------------------
def _engine_keys(cfg):
    from ccedit_amd.config import instantiate_from_config
    with torch.device("meta"):
        engine = instantiate_from_config(cfg.model)
    return engine, {k: list(v.shape) for k, v in engine.state_dict().items()}


def _shipped_model_section(name):
    """The `model:` section of one of the reference's two shipped inference yamls: engine_config() plus the training-time keys
    the shipped files carry on top of it (CLIP legacy_ucg_value "" and freeze, the hint embedder's ucg_rate; the TVI2V file
    also use_checkpoint: True in all three networks and a scheduler_config)."""
    from ccedit_amd.sgm_compat import engine_config
    tvi2v = name == "keyframe_ref_cp_no2ndca_add_cfca_depthzoe.yaml"
    m = engine_config(crossframe=tvi2v)
    emb = m["params"]["conditioner_config"]["params"]["emb_models"]
    emb[0].update(legacy_ucg_value="", params=dict(freeze=True))
    emb[1]["ucg_rate"] = 0.0 if tvi2v else 0.01
    if tvi2v:
        net = m["params"]["network_config"]["params"]
        for p in (net, net["controlnet_config"]["params"], net["controlnet_img_config"]["params"]):
            p["use_checkpoint"] = True
        m["params"]["scheduler_config"] = dict(target="sgm.lr_scheduler.LambdaLinearScheduler", params=dict(
            warm_up_steps=[1000], cycle_lengths=[10000000000000], f_start=[1.e-6], f_max=[1.], f_min=[1.]))
    return m


@pytest.mark.parametrize("name,keys,nparams", [("keyframe_no2ndca_depthmidas.yaml", "keys_tv2v.json", 1608747976),
                                               ("keyframe_ref_cp_no2ndca_add_cfca_depthzoe.yaml", "keys_tvi2v.json", 2171449416)])
def test_shipped_reference_yaml_instantiates_unchanged(tmp_path, golden_dir, name, keys, nparams):
    """the two shipped inference configs load UNCHANGED (legacy_ucg_value: "",
    scheduler_config, use_checkpoint: True, ...) and give the reference's network state-dict names and shapes."""
    import yaml
    from ccedit_amd.config import load_config
    p = tmp_path / name
    p.write_text(yaml.safe_dump(dict(model=_shipped_model_section(name)), sort_keys=False))
    cfg = load_config(str(p))
    engine, mine = _engine_keys(cfg)
    with open(os.path.join(golden_dir, keys)) as f:
        ref = {k: v for k, v in json.load(f).items() if k.startswith("model.")}
    net = {k: v for k, v in mine.items() if k.startswith("model.")}
    assert set(net) == set(ref), (sorted(set(ref) - set(net))[:3], sorted(set(net) - set(ref))[:3])
    assert all(net[k] == ref[k] for k in ref)
    assert sum(int(np.prod(s)) for s in net.values()) == nparams
    clip = engine.conditioner.embedders[0]
    assert clip.legacy_ucg_val == "" and clip.ucg_rate == 0.5 and clip.input_key == "txt"
    assert any(k.startswith("first_stage_model.decoder.") for k in mine)


_INLINE_YAML = """
model:
  target: sgm.models.diffusion.VideoDiffusionEngineTV2V
  params:
    use_ema: False
    scale_factor: 0.18215
    disable_first_stage_autocast: True
    log_keys: [txt]
    freeze_model: spatial
    scheduler_config:
      target: sgm.lr_scheduler.LambdaLinearScheduler
      params: {warm_up_steps: [1000], cycle_lengths: [10000000000000], f_start: [1.e-6], f_max: [1.], f_min: [1.]}
    denoiser_config:
      target: sgm.modules.diffusionmodules.denoiser.DiscreteDenoiser
      params:
        num_idx: 1000
        weighting_config: {target: sgm.modules.diffusionmodules.denoiser_weighting.EpsWeighting}
        scaling_config: {target: sgm.modules.diffusionmodules.denoiser_scaling.EpsScaling}
        discretization_config: {target: sgm.modules.diffusionmodules.discretizer.LegacyDDPMDiscretization}
    network_config:
      target: sgm.modules.diffusionmodules.controlmodel.ControlledUNetModel3DTV2V
      params: &net
        use_checkpoint: True
        in_channels: 4
        out_channels: 4
        model_channels: 32
        attention_resolutions: [4, 2, 1]
        num_res_blocks: 2
        channel_mult: [1, 2, 4, 4]
        num_heads: 2
        use_spatial_transformer: True
        transformer_depth: 1
        context_dim: 64
        legacy: False
        disable_temporal_text_ca: True
        controlnet_config:
          target: sgm.modules.diffusionmodules.controlmodel.ControlNet2D
          params: {use_checkpoint: True, in_channels: 4, hint_channels: 3, model_channels: 32, attention_resolutions: [4, 2, 1],
                   num_res_blocks: 2, channel_mult: [1, 2, 4, 4], num_heads: 2, use_spatial_transformer: True,
                   transformer_depth: 1, context_dim: 64, legacy: False, control_scales: 1.0}
    conditioner_config:
      target: sgm.modules.GeneralConditioner
      params:
        emb_models:
          - is_trainable: False
            input_key: txt
            ucg_rate: 0.5
            legacy_ucg_value: ""
            target: sgm.modules.encoders.modules.FrozenCLIPEmbedder
            params: {freeze: true}
          - is_trainable: False
            input_key: control_hint
            ucg_rate: 0.0
            target: sgm.modules.encoders.modules.DepthMidasEncoder
    first_stage_config:
      target: sgm.models.autoencoder.AutoencoderKLInferenceWrapper
      params:
        embed_dim: 4
        monitor: val/rec_loss
        ddconfig: {double_z: true, z_channels: 4, resolution: 256, in_channels: 3, out_ch: 3, ch: 32, ch_mult: [1, 2, 4, 4],
                   num_res_blocks: 2, attn_resolutions: [], dropout: 0.0}
        lossconfig: {target: torch.nn.Identity}
"""


def test_yaml_with_training_time_keys_loads(tmp_path):
    """Same key set as the shipped yamls (legacy_ucg_value: "", ucg_rate 0.5, scheduler_config, use_checkpoint True) at a
    small width — runs wherever the reference checkout is absent.  ucg settings are stored, and inert at inference:
    get_unconditional_conditioning zeroes ucg_rate around both passes (encoders/modules.py:220-233)."""
    from ccedit_amd.config import load_config
    p = tmp_path / "cfg.yaml"
    p.write_text(_INLINE_YAML)
    engine, mine = _engine_keys(load_config(str(p)))
    emb = engine.conditioner.embedders
    assert emb[0].legacy_ucg_val == "" and emb[0].ucg_rate == 0.5 and emb[1].legacy_ucg_val is None
    seen = []
    for e in emb:
        e.forward = (lambda e_: (lambda x: (seen.append(e_.ucg_rate), x)[1]))(e)
    batch = {"txt": torch.zeros(1, 77, 768), "control_hint": torch.zeros(1, 3, 2, 8, 8)}
    c, uc = engine.conditioner.get_unconditional_conditioning(batch, batch_uc=batch)
    assert seen == [0.0] * 4 and emb[0].ucg_rate == 0.5
    assert set(c) == set(uc) == {"crossattn", "control_hint"}


def test_depth_encoder_refuses_rgb_frames():
    """the reference feeds RGB keyframes to the depth embedder; this build has no depth network, so a tensor
    that looks like RGB must raise instead of reaching the ControlNet as 'depth'."""
    from sgm.modules.encoders.modules import DepthMidasEncoder, DepthZoeEncoder
    for cls in (DepthMidasEncoder, DepthZoeEncoder):
        enc = cls()
        enc.input_key = "control_hint"
        depth = torch.rand(1, 1, 2, 8, 8) * 2 - 1
        hint = depth.repeat(1, 3, 1, 1, 1)
        assert enc(hint) is hint                                   # finished hint: three copies of one map
        assert enc(depth).shape == (1, 3, 2, 8, 8)                  # raw depth: normalised + replicated
        with pytest.raises(NotImplementedError, match="RGB"):
            enc(torch.rand(1, 3, 2, 8, 8))


def test_cfg_cat_cache_is_identity_keyed():
    """ADVICE r1 / VERDICT weak: the (uc, c) concat cache must not serve clip 1's tensor to clip 2 when the allocator hands
    clip 2 the same address — entries hold their sources and are matched by identity + in-place version."""
    from ccedit_amd.sampling import VanillaCFGTV2V
    g = VanillaCFGTV2V(scale=7.5)
    x, s = torch.zeros(1, 4, 2, 4, 4), torch.ones(1)
    mk = lambda v: {"crossattn": torch.full((1, 3, 4), float(v)), "control_hint": torch.full((1, 3, 2, 8, 8), float(v))}
    c1, u1 = mk(1), mk(2)
    out1 = g.prepare_inputs(x, s, c1, u1)[2]
    assert g.prepare_inputs(x, s, c1, u1)[2]["control_hint"] is out1["control_hint"]          # same clip: cached
    # a second clip whose tensors alias the first clip's STORAGE (what address reuse looks like) but are other objects
    c2 = {k: v.view_as(v) for k, v in c1.items()}
    for v in c2.values():
        v.add_(10.0)                                                                           # and other contents
    out2 = g.prepare_inputs(x, s, c2, u1)[2]
    assert out2["control_hint"] is not out1["control_hint"]
    assert float(out2["control_hint"][1].mean()) == 11.0 and float(out2["control_hint"][0].mean()) == 2.0
    # in-place edit of the same object: the version bump invalidates too
    c2["control_hint"].mul_(0.0)
    assert float(g.prepare_inputs(x, s, c2, u1)[2]["control_hint"][1].abs().max()) == 0.0


def _write_toy_clip_tokenizer(d):
    """A structurally valid CLIP BPE vocabulary (byte alphabet, a few merges, the two special tokens) — NOT the real one:
    the ids mean nothing to the trained encoder, the point is the string -> (B,77) int64 plumbing."""
    # the byte alphabet of byte-level BPE: printable bytes map to themselves, the rest to code points from 256 up
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    chars, extra = [], 0
    for b in range(256):
        if b in keep:
            chars.append(chr(b))
        else:
            chars.append(chr(256 + extra))
            extra += 1
    vocab = {}
    for c in chars:
        vocab[c] = len(vocab)
    for c in chars:
        vocab[c + "</w>"] = len(vocab)
    merges = [("c", "a"), ("ca", "t</w>")]
    for a, b in merges:
        vocab[a + b] = len(vocab)
    vocab["<|startoftext|>"] = len(vocab)
    vocab["<|endoftext|>"] = len(vocab)
    with open(os.path.join(d, "vocab.json"), "w") as f:
        json.dump(vocab, f)
    with open(os.path.join(d, "merges.txt"), "w") as f:
        f.write("#version: 0.2\n" + "\n".join(f"{a} {b}" for a, b in merges) + "\n")
    return vocab


def test_clip_tokenizer_path_plumbing(tmp_path, monkeypatch):
    """VERDICT r1 missing #3: prompts as strings.  The vocabulary of openai/clip-vit-large-patch14 is not available offline, so a
    toy vocabulary of the same format stands in: `tokenizer_path` (ctor), CCEDIT_CLIP_TOKENIZER and the scripts' --tokenizer_path
    all reach CLIPTokenizer.from_pretrained, and strings come out as the reference's (B,77) padded id rows
    (encoders/modules.py:396-404: truncation, max_length 77, padding='max_length')."""
    pytest.importorskip("transformers")
    from sgm.modules.encoders.modules import FrozenCLIPEmbedder
    vocab = _write_toy_clip_tokenizer(str(tmp_path))
    with pytest.raises(NotImplementedError, match="tokenizer_path"):       # production guard: only the real 49408-entry vocabulary
        FrozenCLIPEmbedder(tokenizer_path=str(tmp_path)).tokenize(["a cat"])
    monkeypatch.setattr(FrozenCLIPEmbedder, "_expected_vocab", None)        # the toy vocabulary stands in from here on
    emb = FrozenCLIPEmbedder(tokenizer_path=str(tmp_path))
    ids = emb.tokenize(["a cat", "cat " * 100])
    assert ids.shape == (2, 77) and ids.dtype == torch.int64
    bos, eos = vocab["<|startoftext|>"], vocab["<|endoftext|>"]
    assert ids[0, 0] == bos and ids[0, 1] == vocab["a</w>"] and ids[0, 2] == vocab["cat</w>"] and ids[0, 3] == eos
    assert (ids[0, 3:] == eos).all()                                   # CLIP pads with the end-of-text token
    assert ids[1, 0] == bos and ids[1, 76] == eos and (ids[1, 1:76] == vocab["cat</w>"]).all()      # truncated to 77
    monkeypatch.setenv("CCEDIT_CLIP_TOKENIZER", str(tmp_path))
    assert torch.equal(FrozenCLIPEmbedder().tokenize(["a cat"]), ids[:1])
    monkeypatch.delenv("CCEDIT_CLIP_TOKENIZER")
    with pytest.raises(NotImplementedError, match="tokenizer_path"):
        FrozenCLIPEmbedder(version="openai/clip-vit-large-patch14").tokenize(["a cat"])
    # the script composes the strings as the reference does and hands them to the conditioner
    import argparse
    from scripts.sampling.sampling_tv2v import add_common_args, text_inputs
    p = argparse.ArgumentParser()
    add_common_args(p)
    args = p.parse_args(["--prompt", "a cat", "--tokenizer_path", str(tmp_path)])
    assert text_inputs({}, "cpu", args) == (["masterpiece, high quality, a cat"], ["ugly, low quality"])


def test_policy_legacy_environment_values_are_lenient_and_malformed_policy_names_itself():
    """the pre-round-5 one-variable-per-switch spelling treated any string other than "0" as on; such values
    (CCEDIT_GRAPH="", "off", "true") must not fail the import with int()'s ValueError.  A malformed CCEDIT_POLICY entry is an error
    that names the switch."""
    import os
    import subprocess
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    code = "from ccedit_amd import policy; print(policy.get('graph'), policy.get('ff320'), policy.get('lnf'), policy.get('g8_split'))"
    env = dict(os.environ, PYTHONPATH=root, CCEDIT_GRAPH="", CCEDIT_FF320="off", CCEDIT_LNF="true", CCEDIT_G8_SPLIT="3")
    env.pop("CCEDIT_POLICY", None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    assert r.stdout.split() == ["1", "0", "1", "3"]
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=root, CCEDIT_POLICY="graph=yes"), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "graph" in r.stderr and "not an integer" in r.stderr


@pytest.mark.parametrize("name,keys,nparams", [("tv2v_depthmidas.yaml", "keys_tv2v.json", 1608747976), ("tvi2v_ref_depthzoe.yaml", "keys_tvi2v.json", 2171449416)])
def test_generated_yamls_build_the_reference_state_dict(tmp_path, golden_dir, name, keys, nparams):
    """VERDICT r5, missing 6: no inference yaml travelled with the repo, so "the shipped yamls load" was only testable beside the
    reference tree.  tools/make_configs.py writes the two configurations of the path from sgm_compat.engine_config(); loaded through
    load_config + instantiate_from_config (the entry points' route) they give the reference's network state-dict names, shapes and
    parameter count — wherever this runs."""
    import subprocess
    import sys
    from ccedit_amd.config import load_config
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "make_configs.py"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    cfg = load_config(str(tmp_path / name))
    assert cfg.model.params.disable_first_stage_autocast is True          # what selects the fp32 first stage (policy vae_fp32 = 2)
    engine, mine = _engine_keys(cfg)
    with open(os.path.join(golden_dir, keys)) as f:
        ref = {k: v for k, v in json.load(f).items() if k.startswith("model.")}
    net = {k: v for k, v in mine.items() if k.startswith("model.")}
    assert set(net) == set(ref), (sorted(set(ref) - set(net))[:3], sorted(set(net) - set(ref))[:3])
    assert all(net[k] == ref[k] for k in ref)
    assert sum(int(np.prod(s_)) for s_ in net.values()) == nparams
    assert engine.first_stage_model.precision == "fp32"


def test_bench_reads_traffic_from_the_capture_of_this_build(tmp_path, monkeypatch):
    """bench.py's `roofline.traffic` comes from the committed PMC capture whose `kernel_source_hash` is THIS build's (the newest round's
    file otherwise, reported as stale): a fixed file name silently went stale when a later round re-captured (round 6)."""
    import json
    import bench
    prof = tmp_path / "profiles"
    prof.mkdir()
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    monkeypatch.setattr(bench, "kernel_source_hash", lambda: "abc")
    assert bench.pmc_traffic_file() == "r06_pmc_traffic.json"                      # nothing there: the name the note will mention
    (prof / "r04_pmc_traffic.json").write_text(json.dumps({"kernel_source_hash": "abc"}))
    (prof / "r05_pmc_traffic.json").write_text(json.dumps({"kernel_source_hash": "old"}))
    (prof / "r05_pmc_traffic_tvi2v.json").write_text(json.dumps({"kernel_source_hash": "abc"}))
    assert bench.pmc_traffic_file() == "r04_pmc_traffic.json"                      # the matching capture wins over the newer stale one
    assert bench.pmc_traffic_file(True) == "r05_pmc_traffic_tvi2v.json"
    (prof / "r04_pmc_traffic.json").write_text("not json")
    assert bench.pmc_traffic_file() == "r05_pmc_traffic.json"                      # no match: the newest file (bench.py reports it stale)
