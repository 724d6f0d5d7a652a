"""A text context per frame — cond['crossattn'] of shape (B*T, L, C) in (b t) order — through the network on a real MI355X, on the
reduced-width synthetic network of the region / window tests: the transformer block against the oracle's basic_block (which takes one
row block of context per frame already), the whole wrapper against the plain form, graphs, caches and windows."""
import pytest
import torch

pytestmark = pytest.mark.gpu

G160 = dict(model_channels=160, num_heads=4, context_dim=128)
NET_TOL = 3e-2            # tests/test_network_gpu.py: one network evaluation against the fp32 oracle
BLOCK_TOL_ATTN = 9e-3     # tests/test_network_gpu.py: one block with attention against the bf16-emulating oracle on the oracle's input
B, T, H, W = 2, 3, 8, 8


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


@pytest.fixture(scope="module")
def g160_wrapper():
    _need_gpu()
    from ccedit_amd.sgm_compat import build_network
    from ccedit_amd.utils.synth import fill_module_
    w = build_network("cpu", **G160)
    fill_module_(w, prefix="model.")
    w.diffusion_model.pack("cuda")
    return w


@pytest.fixture(scope="module")
def inputs():
    g = torch.Generator().manual_seed(2024)
    x1 = torch.randn(1, 4, T, H, W, generator=g)
    hint = torch.rand(1, 3, T, 8 * H, 8 * W, generator=g) * 2 - 1
    clip_ctx = torch.randn(B, 77, 128, generator=g)                      # (uc, c): one context per clip
    frame_ctx = torch.randn(B * T, 77, 128, generator=g)                 # one per frame, all different
    t = torch.tensor([433, 433], dtype=torch.int64)
    return dict(x=torch.cat([x1, x1]).cuda(), hint=hint.repeat(2, 1, 1, 1, 1).cuda(), clip_ctx=clip_ctx.cuda(), frame_ctx=frame_ctx.cuda(),
                t=t.cuda())


class _eager:
    """The wrapper without graphs and with empty caches, put back as found."""

    def __init__(self, w, use_graph=False):
        self.w, self.use_graph = w, use_graph

    def __enter__(self):
        self.saved = (self.w.use_graph, self.w.cache_state())
        self.w.use_graph = self.use_graph
        self.w.reset_caches()
        return self.w

    def __exit__(self, *exc):
        self.w.use_graph = self.saved[0]
        self.w.reset_caches()
        self.w.restore_cache_state(self.saved[1])


# ---- 1. the block ----------------------------------------------------------------------------------
def test_block_with_a_context_per_frame_vs_oracle(g160_wrapper):
    """BasicTransformerBlock.run on B*T = 6 frames with six different contexts against oracle.basic_block under bf16 emulation, with the
    bound of the teacher-forced per-block test; with the shared CFG prefix (one half in, both halves out) as well."""
    from ccedit_amd import hip, network
    from ccedit_amd.sgm_compat import build_network_spec
    from ccedit_amd.utils.synth import synth_state_dict
    from oracle import ccedit_oracle as O
    net = g160_wrapper.diffusion_model
    j, st = next((j, m) for j, m in enumerate(net.input_blocks[1]) if isinstance(m, network.SpatialTransformer))
    blk = st.transformer_blocks[0]
    p = f"model.diffusion_model.input_blocks.1.{j}.transformer_blocks.0"
    sd = synth_state_dict(build_network_spec(G160))
    dim, heads, hw = blk.attn1.inner, blk.attn1.heads, H * W
    g = torch.Generator().manual_seed(7)
    half = torch.randn(T * hw, dim, generator=g).to(torch.bfloat16)                          # one CFG half; its twin is identical
    tok = torch.cat([half, half])
    ctx = torch.randn(B * T, 77, 128, generator=g).to(torch.bfloat16)
    with O.bf16_emulation():
        want = O.basic_block(sd, p, tok.float().view(B * T, hw, dim), ctx.float(), heads)
    ctx2d = ctx.reshape(-1, 128).contiguous().cuda()
    full = blk.run(tok.cuda(), B * T, hw, ctx2d, 77, T)
    label = hip.lib().ccedit_last_kernel().decode()
    shared = blk.run(half.cuda(), B * T, hw, ctx2d, 77, T, shared=True)
    r_f, r_s, d = _rel(full.view(B * T, hw, dim), want), _rel(shared.view(B * T, hw, dim), want), _rel(shared, full)
    print(f"per-frame context, block {p}: vs bf16-emulating oracle {r_f:.4f} (shared prefix {r_s:.4f}); shared vs full {d:.4f}; last kernel {label}")
    assert r_f < BLOCK_TOL_ATTN and r_s < BLOCK_TOL_ATTN and d < r_f + r_s
    # the contexts matter frame by frame: frame 4's context given to every frame is another result in every other frame
    same = ctx[4:5].expand(B * T, -1, -1).reshape(-1, 128).contiguous().cuda()
    moved = blk.run(tok.cuda(), B * T, hw, same, 77, T).view(B * T, hw, dim)
    fv = full.view(B * T, hw, dim)
    assert torch.equal(moved[4], fv[4]) and all(not torch.equal(moved[f], fv[f]) for f in (0, 1, 2, 3, 5))
    with pytest.raises(ValueError, match="text context of 308 rows: expected 2 clips or 6 frames of 77 rows"):
        blk.run(tok.cuda(), B * T, hw, ctx2d[: 4 * 77], 77, T)


# ---- 2. the wrapper ----------------------------------------------------------------------------------
def test_repeated_context_per_frame_gives_the_plain_evaluation(g160_wrapper, inputs):
    """Every clip's context repeated for its T frames is the plain (B, L, C) evaluation computed another way (kv_div = 1, the general
    attention kernels): both are within NET_TOL of the oracle, so they are within 2 NET_TOL of each other."""
    i = inputs
    rep = i["clip_ctx"].repeat_interleave(T, dim=0).contiguous()
    with _eager(g160_wrapper) as w:
        plain = w(i["x"], i["t"], dict(crossattn=i["clip_ctx"], control_hint=i["hint"]))
        per_frame = w(i["x"], i["t"], dict(crossattn=rep, control_hint=i["hint"]))
    r = _rel(per_frame, plain)
    print(f"context repeated per frame vs plain (B, L, C): rel rms {r:.5f} (bound {2 * NET_TOL})")
    assert bool(torch.isfinite(per_frame).all()) and r <= 2 * NET_TOL


def test_varying_context_changes_the_result_reruns_bit_equal_and_replays(g160_wrapper, inputs):
    i = inputs
    c_plain = dict(crossattn=i["clip_ctx"], control_hint=i["hint"])
    c_frame = dict(crossattn=i["frame_ctx"], control_hint=i["hint"])
    w = g160_wrapper
    before = (w.use_graph, w._graph_slots, w._hint_slots, w._tkv_slots, w._windows, w._contexts)
    with _eager(w):
        plain = w(i["x"], i["t"], c_plain)
        eager = w(i["x"], i["t"], c_frame)
        assert bool(torch.isfinite(eager).all()) and _rel(eager, plain) > 1e-2, "six different contexts changed nothing"
        assert torch.equal(w(i["x"], i["t"], c_frame), eager)
        assert len(w._tkv_val) == 4                                      # (UNet, ControlNet) x (plain, per frame): kept per tensor as today
    with _eager(w, use_graph=True):
        w.graph_counts = None
        outs = [w(i["x"], i["t"], c_frame) for _ in range(3)]            # eager, capture + replay, replay
        assert not type(w)._graph_failed and w.graph_counts == dict(eager=1, capture=1, replay=1)
        assert all(torch.equal(o, eager) for o in outs), "a replay through the captured graph differs from the eager evaluation"
    assert before == (w.use_graph, w._graph_slots, w._hint_slots, w._tkv_slots, w._windows, w._contexts)
    assert not w._graphs and not w._tkv_val


def test_wrong_leading_size_is_refused(g160_wrapper, inputs):
    i = inputs
    with _eager(g160_wrapper) as w:
        for n in (3, 4, 12):
            with pytest.raises(ValueError, match=rf"crossattn \({n}, 77, 128\): expected \(2, L, C\), one context per clip, or \(6, L, C\), one per frame"):
                w(i["x"], i["t"], dict(crossattn=torch.zeros(n, 77, 128, device="cuda"), control_hint=i["hint"]))
    net = g160_wrapper.diffusion_model
    with pytest.raises(ValueError, match="one context per clip"):
        net(i["x"], i["t"], context=torch.zeros(4, 77, 128, device="cuda"), control=[torch.zeros(1)])
    with pytest.raises(ValueError, match="one context per clip"):
        net.controlnet(i["x"], i["hint"], i["t"], torch.zeros(4, 77, 128, device="cuda"))


# ---- 3. windows --------------------------------------------------------------------------------------
def test_one_window_is_the_unwindowed_evaluation_and_windows_get_their_frames_contexts(g160_wrapper, inputs):
    from ccedit_amd import ops
    from ccedit_amd.windows import WindowedDenoiser, plan
    i = inputs
    w = g160_wrapper
    sigma = torch.ones(2)

    def denoiser(x, s, c):
        return w(x, i["t"], c)
    with _eager(w):
        c_frame = dict(crossattn=i["frame_ctx"], control_hint=i["hint"])
        direct = denoiser(i["x"], sigma, c_frame)
        wd = WindowedDenoiser(denoiser, T, wrapper=w)
        assert torch.equal(wd(i["x"], sigma, c_frame), direct)           # N == T: one window, the wrapped closure's own bits
        assert w._tkv_slots == 6
        # N = 5 in windows of 3: every window sees the contexts of ITS frames
        n = 5
        g = torch.Generator().manual_seed(9)
        x1 = torch.randn(1, 4, n, H, W, generator=g)
        xl = torch.cat([x1, x1]).cuda()
        hint = (torch.rand(1, 3, n, 8 * H, 8 * W, generator=g) * 2 - 1).repeat(2, 1, 1, 1, 1).cuda()
        ctx = torch.randn(B * n, 77, 128, generator=g).cuda()
        wd = WindowedDenoiser(denoiser, T, overlap=1, wrapper=w)
        got = wd(xl, sigma, dict(crossattn=ctx, control_hint=hint))
        starts, coef = plan(n, T, 1)
        assert len(starts) == 2 and (w._graph_slots, w._tkv_slots, w._window_contexts) == (2, 6, True)
        assert torch.equal(wd(xl, sigma, dict(crossattn=ctx, control_hint=hint)), got)
        ys = []
        for s in starts:
            ci = dict(crossattn=ctx.view(B, n, 77, 128)[:, s:s + T].reshape(B * T, 77, 128).contiguous(),
                      control_hint=hint[:, :, s:s + T].contiguous())
            ys.append(denoiser(xl[:, :, s:s + T].contiguous(), sigma, ci).float().contiguous())
        want = ops.window_fuse(ys, torch.tensor(starts, dtype=torch.int32).cuda(), torch.from_numpy(coef).cuda(), n)
        assert torch.equal(got, want)
        w.reserve_windows(0)
