"""Long and weighted prompts on a real MI355X (ccedit_amd/prompt.py, csrc/prompt.hip, --prompt_chunks / --prompt_syntax).

Exact (no tolerance): `ccedit_prompt_weight` against the numpy restatement of its definition (tests/_prompt_numpy.py); `encode_long`
against one call of the text transformer on the (B n, 77) view; a 77-row context before and after a longer one; the files of a job
with a short plain prompt with and without the flags.  Against the fp32 CPU oracle: every chunk of `encode_long`, and one network
evaluation with a context of 154 and of 308 rows, each with the budget of the existing one-evaluation tests (NET_TOL)."""
import glob
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _prompt_cases as PC  # noqa: E402
import _prompt_numpy as PN  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
G160 = dict(model_channels=160, num_heads=4, context_dim=128)
NET_TOL = 3e-2       # relative RMS, one network evaluation / one text-encoder call (tests/test_network_gpu.py)
WEIGHTS = np.array([0, 0.5, 1, 1.1, 1.21, 8], np.float32)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


def _bits(t):
    if torch.is_tensor(t):
        t = t.detach().cpu().contiguous().numpy()
    return np.ascontiguousarray(t).view(np.int32)


# ---- 1. the kernel ---------------------------------------------------------------------------------
def _zew(b, n, c, seed):
    """z with entries at both ends of the fp32 range, e, and weights drawn from the issue's set (every value present)."""
    rs = np.random.RandomState(seed)
    z = rs.standard_normal((b, 77 * n, c)).astype(np.float32)
    e = rs.standard_normal((77, c)).astype(np.float32)
    for v in (1e-30, -1e-30, 1e30, -1e30):
        z.reshape(-1)[rs.choice(z.size, 64, replace=False)] = v
    w = rs.choice(WEIGHTS, size=(b, 77 * n)).astype(np.float32)
    w[0, :6] = WEIGHTS
    return z, e, w


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("c", [768, 10])                 # 16-byte accesses; one element per access (C % 4 != 0)
def test_prompt_weight_is_exact(n, c):
    _need_gpu()
    from ccedit_amd import ops
    z, e, w = _zew(2, n, c, 7 * n + c)
    want = PN.prompt_weight(z, e, w)
    zt, et, wt = torch.from_numpy(z).cuda(), torch.from_numpy(e).cuda(), torch.from_numpy(w).cuda()
    got = ops.prompt_weight(zt, et, wt)                                                  # out of place: z is left alone
    assert got.data_ptr() != zt.data_ptr() and np.array_equal(_bits(zt), _bits(z))
    assert np.array_equal(_bits(got), _bits(want))
    buf = zt.clone()
    assert ops.prompt_weight(buf, et, wt, out=buf) is buf                                # in place
    assert np.array_equal(_bits(buf), _bits(want))
    ones = ops.prompt_weight(zt, et, torch.ones_like(wt))
    assert torch.equal(ones, zt)                                                         # w == 1: z's bits
    zero = ops.prompt_weight(zt, et, torch.zeros_like(wt))
    assert np.array_equal(_bits(zero), _bits(PN.prompt_weight(z, e, np.zeros_like(w))))


def test_prompt_weight_copies_nan_rows_of_weight_one_and_reads_unaligned_tensors():
    _need_gpu()
    from ccedit_amd import ops
    z, e, w = _zew(2, 1, 12, 3)
    z[0, 5, :] = np.float32(np.nan)
    w[0, 5] = 1.0
    base = torch.zeros(z.size + 1, dtype=torch.float32, device="cuda")
    zt = base[1:].view(z.shape)                                                          # 4-byte aligned only
    zt.copy_(torch.from_numpy(z))
    got = ops.prompt_weight(zt, torch.from_numpy(e).cuda(), torch.from_numpy(w).cuda())
    assert np.array_equal(_bits(got), _bits(PN.prompt_weight(z, e, w)))


def test_prompt_weight_refuses_bad_arguments():
    _need_gpu()
    from ccedit_amd import ops
    z, e, w = (torch.from_numpy(v).cuda() for v in _zew(1, 2, 8, 1))
    for bad in (float("nan"), float("inf")):
        w2 = w.clone()
        w2[0, 100] = bad
        with pytest.raises(ValueError, match="NaN or infinite"):
            ops.prompt_weight(z, e, w2)
    with pytest.raises(ValueError, match="expected"):
        ops.prompt_weight(z[:, :100].contiguous(), e, w[:, :100].contiguous())
    with pytest.raises(ValueError, match="expected"):
        ops.prompt_weight(z, e[:76].contiguous(), w)
    with pytest.raises(ValueError, match="contiguous cuda fp32"):
        ops.prompt_weight(z.double(), e, w)


# ---- 2. encode_long ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clip_embedder():
    _need_gpu()
    from ccedit_amd.config import instantiate_from_config
    from ccedit_amd.utils.synth import fill_module_
    emb = instantiate_from_config(dict(target="sgm.modules.encoders.modules.FrozenCLIPEmbedder", params=dict(freeze=True)))
    fill_module_(emb, prefix="conditioner.embedders.0.")
    emb.pack("cuda")
    return emb


def _chunk_ids(b, n, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 49406, (b, 77 * n), generator=g)
    ids.view(b * n, 77)[:, 0] = 49406
    ids.view(b * n, 77)[:, 60:] = 49407
    return ids


def test_encode_long_is_the_transformer_on_the_chunk_view(clip_embedder, golden_dir):
    from ccedit_amd.utils.synth import synth_state_dict
    from oracle import ccedit_oracle as O
    emb = clip_embedder
    ids = _chunk_ids(2, 3, 11)
    out = emb.encode_long(ids.cuda())
    assert out.shape == (2, 231, 768) and out.dtype == torch.float32
    rows = emb.transformer(ids.view(6, 77).cuda())
    assert torch.equal(out, rows.view(2, 231, 768))
    with open(os.path.join(golden_dir, "keys_clip_text.json")) as f:
        sd = synth_state_dict([(k, tuple(v)) for k, v in json.load(f).items()])
    ref = O.clip_text_forward(sd, "conditioner.embedders.0.transformer.text_model", O.CLIPTextConfig(), ids.view(6, 77)).view(2, 3, 77, 768)
    errs = [_rel(out.view(2, 3, 77, 768)[b, k], ref[b, k]) for b in range(2) for k in range(3)]
    print("encode_long rel rms err per chunk vs oracle:", ["%.4f" % v for v in errs])
    assert max(errs) < NET_TOL, errs
    # forward for (B, 77) is what it was: one chunk through encode_long is forward's result
    assert torch.equal(emb.encode_long(ids[:, :77].cuda()), emb(ids[:, :77].cuda()))
    with pytest.raises(ValueError, match="chunks of 77"):
        emb.encode_long(ids[:, :78].cuda())


def test_encode_long_weights_interpolate_from_the_empty_chunk(clip_embedder):
    emb = clip_embedder
    ids = _chunk_ids(2, 2, 12)
    z = emb.encode_long(ids.cuda())
    e = emb.empty_chunk_encoding()
    assert e.shape == (77, 768) and emb.empty_chunk_encoding() is e                       # computed once
    assert torch.equal(e, emb.transformer(torch.tensor([[49406] + [49407] * 76]).cuda())[0])
    assert torch.equal(emb.encode_long(ids.cuda(), torch.ones(2, 154)), z)                # weight 1 everywhere: the unweighted encoding
    w = torch.from_numpy(np.random.RandomState(2).choice(WEIGHTS, size=(2, 154)).astype(np.float32))
    got = emb.encode_long(ids.cuda(), w)
    want = PN.prompt_weight(z.cpu().numpy(), e.cpu().numpy(), w.numpy())
    assert np.array_equal(_bits(got), _bits(want))
    zero = emb.encode_long(ids.cuda(), torch.zeros(2, 154))
    assert torch.equal(zero, e.repeat(2, 1)[None].expand(2, -1, -1))


# ---- 3. one evaluation of the network with 77 n rows of context ----------------------------------------
@pytest.fixture(scope="module")
def g160_wrapper():
    _need_gpu()
    from ccedit_amd.sgm_compat import build_network
    from ccedit_amd.utils.synth import fill_module_
    w = build_network("cpu", **G160)
    fill_module_(w, prefix="model.")
    w.diffusion_model.pack("cuda")
    return w


def _eval_inputs(rows, seed, latent=(8, 8), frames=3):
    """A CFG-doubled evaluation: identical halves of the latent, two contexts of `rows` rows."""
    g = torch.Generator().manual_seed(seed)
    h, w = latent
    x = torch.randn(1, 4, frames, h, w, generator=g).repeat(2, 1, 1, 1, 1)
    hint = (torch.rand(1, 1, frames, 8 * h, 8 * w, generator=g) * 2 - 1).repeat(2, 3, 1, 1, 1)
    c = dict(crossattn=torch.randn(2, rows, 128, generator=g), control_hint=hint)
    return x, torch.tensor([17, 17], dtype=torch.int64), c


@pytest.mark.parametrize("rows", [154, 308])
def test_network_eval_with_a_long_context_vs_oracle(g160_wrapper, rows):
    from ccedit_amd.sgm_compat import build_network_spec
    from ccedit_amd.utils.synth import synth_state_dict
    from oracle import ccedit_oracle as O
    x, t, c = _eval_inputs(rows, rows)
    ref = O.network_forward(synth_state_dict(build_network_spec(G160)), O.NetConfig(**G160), x, t, c)
    g160_wrapper.reset_caches()
    eps = g160_wrapper(x.cuda(), t.cuda(), {k: v.cuda() for k, v in c.items()})
    r = _rel(eps, ref)
    print(f"network eval, context of {rows} rows: rel rms err vs oracle {r:.4f}")
    assert eps.shape == x.shape and bool(torch.isfinite(eps).all())
    assert r < NET_TOL, r
    # the extra rows matter: the same evaluation on the first 77 rows alone is another result
    short = g160_wrapper(x.cuda(), t.cuda(), dict(crossattn=c["crossattn"][:, :77].contiguous().cuda(), control_hint=c["control_hint"].cuda()))
    assert _rel(short, eps) > 1e-3


@pytest.mark.parametrize("rows", [154, 308])
def test_a_long_context_replays_its_graph_and_keeps_the_text_cache(g160_wrapper, rows):
    """Four evaluations with the same conditioning tensors: one eager, one captured, two replayed; the text K / V projection of each
    network ran once (the cache is keyed by the context tensor, whatever its length); all four give the same bits."""
    w = g160_wrapper
    if not w.use_graph:
        pytest.skip("HIP graphs are switched off by policy")
    nets = (w.diffusion_model, w.diffusion_model.controlnet)
    calls = {id(n): 0 for n in nets}

    def counting(net):
        inner = type(net).text_kv.__get__(net)

        def text_kv(ctx2d):
            calls[id(net)] += int(torch.is_tensor(ctx2d))      # (run() hands a finished TextKV through the same method: no projection)
            return inner(ctx2d)
        return text_kv

    x, t, c = _eval_inputs(rows, 3 + rows, latent=(16, 24))
    x, t = x.cuda(), t.cuda()
    c = {k: v.cuda() for k, v in c.items()}
    try:
        for n in nets:
            n.text_kv = counting(n)
        w.reset_caches()
        w.reserve_windows(0)
        outs = [w(x, t, c).clone() for _ in range(4)]
        assert dict(w.graph_counts) == dict(eager=1, capture=1, replay=2), dict(w.graph_counts)
        assert [calls[id(n)] for n in nets] == [1, 1], [calls[id(n)] for n in nets]
        assert len(w._tkv_val) == 2 and len(w._graphs) == 1 and all(e.captured for e in w._graphs.values())
        kv = next(iter(w._tkv_val.values()))
        assert kv.kv_all is not None and kv.kv_all.shape[0] == 2 * rows                  # ONE GEMM projected all 77 n rows of both halves
        assert all(torch.equal(o, outs[0]) for o in outs[1:])
    finally:
        for n in nets:
            n.__dict__.pop("text_kv", None)
        w.reserve_windows(0)


def test_a_77_row_context_is_untouched_by_a_longer_one_between(g160_wrapper):
    w = g160_wrapper
    x, t, c77 = _eval_inputs(77, 21, latent=(16, 24))
    _, _, c154 = _eval_inputs(154, 22, latent=(16, 24))
    x, t = x.cuda(), t.cuda()
    c77 = {k: v.cuda() for k, v in c77.items()}
    c154 = dict(crossattn=c154["crossattn"].cuda(), control_hint=c77["control_hint"])
    w.reset_caches()
    before = [w(x, t, c77).clone() for _ in range(3)]                                    # eager, captured, replayed
    long = [w(x, t, c154).clone() for _ in range(3)]
    after = [w(x, t, c77).clone() for _ in range(3)]
    assert all(torch.equal(v, before[0]) for v in before[1:] + after)
    assert all(torch.equal(v, long[0]) for v in long[1:]) and not torch.equal(long[0], before[0])


# ---- 4. entry point ------------------------------------------------------------------------------
def _write_config(tmp_path):
    import yaml
    from ccedit_amd.sgm_compat import engine_config
    cfg = os.path.join(str(tmp_path), "tv2v.yaml")
    with open(cfg, "w") as f:       # the text encoder's width: prompts go through the tokenizer and the CLIP model
        yaml.safe_dump(dict(model=engine_config(crossframe=False, vae_ch=32, model_channels=64, num_heads=2, context_dim=768)), f)
    return cfg


@pytest.fixture()
def clip(tmp_path, monkeypatch):
    """A 64 x 128 frame directory of 9 frames (3 keyframes at 9 -> 3 fps), a half-frame mask image, the toy vocabulary."""
    pytest.importorskip("transformers")
    from PIL import Image
    from sgm.modules.encoders.modules import FrozenCLIPEmbedder
    rs = np.random.RandomState(8)
    vdir = tmp_path / "clips" / "bear"
    vdir.mkdir(parents=True)
    for i in range(9):
        Image.fromarray(rs.randint(0, 256, (64, 128, 3)).astype(np.uint8)).save(str(vdir / f"{i:03d}.png"))
    half = np.zeros((64, 128), np.uint8)
    half[:, 64:] = 255
    Image.fromarray(half).save(str(tmp_path / "half.png"))
    tok = tmp_path / "tok"
    tok.mkdir()
    PC.write_toy_clip_tokenizer(tok)
    monkeypatch.setattr(FrozenCLIPEmbedder, "_expected_vocab", None)
    monkeypatch.setenv("CCEDIT_CLIP_TOKENIZER", str(tok))                                 # (build_model sets it: put back afterwards)
    base = ["--config_path", _write_config(tmp_path), "--synthetic", "--H", "64", "--W", "128", "--num_keyframes", "3", "--sample_steps", "2",
            "--sampler_name", "DPMPP2SAncestralSampler", "--original_fps", "9", "--target_fps", "3", "--noise_seed", "1",
            "--video_path", str(vdir), "--batch_size", "1", "--save_type", "npy", "--tokenizer_path", str(tok)]
    return tmp_path, base


def _job(monkeypatch, base, out, *extra):
    """The job through scripts.sampling.sampling_tv2v.main in this process -> (result file's bytes, log_info)."""
    from scripts.sampling import sampling_tv2v as S
    monkeypatch.setattr(sys, "argv", ["sampling_tv2v.py", *base, "--save_path", out, *extra])
    S.main()
    files = sorted(glob.glob(os.path.join(out, "default", "result", "npy", "frames-*.npy")))
    assert len(files) == 1, files
    with open(os.path.join(out, "default", "log_info.json")) as f:
        return open(files[0], "rb").read(), np.load(files[0]), json.load(f)


LONG = "a (b:1.3) " + PC.words(97) + " [cat]"          # 100 tokens of the toy vocabulary, with emphasis


@pytest.mark.timeout(900)
def test_entry_point_takes_a_long_weighted_prompt(clip, monkeypatch):
    _need_gpu()
    tmp_path, base = clip
    flags = ("--prompt_syntax", "weighted", "--prompt_chunks", "3")
    _, res, log = _job(monkeypatch, base, str(tmp_path / "long"), "--prompt", LONG, "--add_prompt", "", *flags)
    assert res.shape == (3, 64, 128, 3) and np.isfinite(res).all()
    assert log["prompts"] == [dict(prompt_tokens=100, prompt_chunks=2, negative_prompt_tokens=15, negative_prompt_chunks=1, context_rows=154)]
    # what lies past 75 tokens reaches the result: the same job on the first 75 tokens alone is another clip
    _, cut, _ = _job(monkeypatch, base, str(tmp_path / "cut"), "--prompt", "a (b:1.3) " + PC.words(73), "--add_prompt", "", *flags)
    assert not np.array_equal(res, cut)
    with pytest.raises(ValueError, match=r"--prompt: 100 tokens need 2 chunks .* --prompt_chunks is 1"):
        _job(monkeypatch, base, str(tmp_path / "refused"), "--prompt", LONG, "--add_prompt", "", "--prompt_syntax", "weighted")
    assert not os.path.exists(str(tmp_path / "refused" / "default" / "result"))


@pytest.mark.timeout(900)
def test_entry_point_with_a_short_plain_prompt_writes_the_same_bytes_with_and_without_the_flags(clip, monkeypatch):
    _need_gpu()
    tmp_path, base = clip
    with_flags, _, log = _job(monkeypatch, base, str(tmp_path / "new"), "--prompt", "a cat", "--prompt_syntax", "weighted", "--prompt_chunks", "3")
    without, _, plog = _job(monkeypatch, base, str(tmp_path / "old"), "--prompt", "a cat")
    assert log["prompts"][0]["context_rows"] == 77 and log["prompts"][0]["prompt_chunks"] == 1 and "prompts" not in plog
    assert with_flags == without


@pytest.mark.timeout(900)
def test_entry_point_gives_a_region_prompt_of_another_length_the_same_context_length(clip, monkeypatch):
    _need_gpu()
    tmp_path, base = clip
    half = str(tmp_path / "half.png")
    _, res, log = _job(monkeypatch, base, str(tmp_path / "region"), "--prompt", "a cat", "--add_prompt", "", "--prompt_chunks", "3",
                       "--region_prompt", PC.words(160), "--region_mask", half)
    assert res.shape == (3, 64, 128, 3) and np.isfinite(res).all()
    assert log["prompts"] == [dict(prompt_tokens=2, prompt_chunks=1, negative_prompt_tokens=15, negative_prompt_chunks=1, context_rows=231)]
    assert log["regions"][0]["prompt"] == PC.words(160)
