"""Full-frame-rate output on a real MI355X (ccedit_amd/propagate.py, csrc/propagate.hip, --propagate).

Exact (no tolerance anywhere): every entry point and propagate_clip as a whole against the numpy restatement
(tests/_propagate_numpy.py, whose own properties tests/test_propagate.py checks) on random bytes and on structured scenes — an object
moving over a moving background — at 64 x 64, 128 x 192 and one 512 x 768 pair, gaps 1, 2 and 7, two keyframes and six.  Also: the
result does not depend on the pair chunking, device tables and pair lists are clamped and not followed, bad arguments are reported,
and the entry point end to end (--synthetic, a small frame directory)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _propagate_numpy as ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SIZES = [(64, 64), (128, 192)]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _textured(h, w, seed, smooth=5):
    rs = np.random.RandomState(seed)
    a = rs.randint(0, 256, (h, w, 3)).astype(np.float64)
    k = np.ones(smooth) / smooth
    for ax in (0, 1):
        a = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), ax, a)
    return ((a - a.min()) / (a.max() - a.min()) * 255).astype(np.uint8)


def scene(h, w, frames, seed=0, bg=(1, -2), obj=(-2, 3)):
    """An object (its own texture, a third of the frame) moving by `obj` pixels per frame over a background moving by `bg`."""
    big = _textured(h + 2 * 8 * frames + 32, w + 2 * 8 * frames + 32, seed)
    oh, ow = h // 3, w // 3
    thing = _textured(oh, ow, seed + 1, smooth=3)
    out = []
    for t in range(frames):
        y0, x0 = 8 * frames + bg[0] * t, 8 * frames + bg[1] * t
        f = big[y0:y0 + h, x0:x0 + w].copy()
        oy = int(np.clip(h // 3 + obj[0] * t, 0, h - oh))
        ox = int(np.clip(w // 3 + obj[1] * t, 0, w - ow))
        f[oy:oy + oh, ox:ox + ow] = thing
        out.append(f)
    return np.stack(out)


def random_frames(h, w, frames, seed):
    return np.random.RandomState(seed).randint(0, 256, (frames, h, w, 3)).astype(np.uint8)


def edit(x):
    return np.stack([255 - x[..., 0], x[..., 2], (x[..., 1] // 2 + 64).astype(np.uint8)], axis=-1)


def _pyramids(src):
    return [ref.pyramid(ref.luma(f)) for f in src]


def _pairs(rows):
    return _dev(np.asarray(rows, np.int32).reshape(-1, 4))


# ---- 1. the entry points, one by one ---------------------------------------------------------------
@pytest.mark.parametrize("h,w,frames", [(64, 64, 3), (128, 192, 2), (512, 768, 2)])
def test_pyramid_is_exact(h, w, frames):
    _need_gpu()
    from ccedit_amd import ops
    for src in (random_frames(h, w, frames, 1), scene(h, w, frames, 2)):
        pyr = ops.prop_pyramid(_dev(src))
        want = _pyramids(src)
        for lv in range(4):
            got = ops.prop_level(pyr, frames, h, w, lv).cpu().numpy()
            assert np.array_equal(got, np.stack([p[lv] for p in want])), (h, w, lv)


@pytest.mark.parametrize("h,w", SIZES + [(512, 768)])
@pytest.mark.parametrize("kind", ["random", "scene"])
def test_match_is_exact_on_every_level(h, w, kind):
    """Every level against the restatement, each fed the restatement's own parent vectors, and the chain of four as a whole.  Pairs:
    (0 -> 2), (1 -> 0), (1 -> 2) (one pair only at 512 x 768)."""
    _need_gpu()
    from ccedit_amd import ops
    from ccedit_amd.propagate import device_tables, match_pairs, radius_of
    src = random_frames(h, w, 3, 3) if kind == "random" else scene(h, w, 3, 4, bg=(2, -3), obj=(-5, 6))
    rows = [(0, 2, 0, 1)] if h == 512 else [(0, 2, 0, 1), (1, 0, 0, 1), (1, 2, 0, 1)]
    pyr_np = _pyramids(src)
    pyr = ops.prop_pyramid(_dev(src))
    pairs = _pairs(rows)
    ranks, _ = device_tables(pyr.device)
    want = [None] * 4
    for lv in (3, 2, 1, 0):
        parents = None
        if lv < 3:
            nby, nbx = (h >> lv) // 8, (w >> lv) // 8
            parents = np.stack([want[lv + 1][i] for i in range(len(rows))])
        level = []
        for i, (f, k, _, _) in enumerate(rows):
            pred = None if parents is None else 2 * parents[i][np.arange(nby)[:, None] >> 1, np.arange(nbx)[None, :] >> 1]
            level.append(ref.match_level(pyr_np[f][lv], pyr_np[k][lv], pred, radius_of(lv)))
        want[lv] = np.stack(level)
        got = ops.prop_match(pyr, pairs, ranks[lv], None if parents is None else _dev(parents.astype(np.int32)), 3, h, w, lv, radius_of(lv))
        assert np.array_equal(got.cpu().numpy(), want[lv]), (kind, h, w, lv, int((got.cpu().numpy() != want[lv]).sum()))
    chain = match_pairs(pyr, pairs, 3, h, w).cpu().numpy()
    assert np.array_equal(chain, want[0])
    for i, (f, k, _, _) in enumerate(rows):
        assert np.array_equal(chain[i], ref.match(pyr_np[f], pyr_np[k]))
    if kind == "scene":
        assert np.abs(chain).max() > 0, "the scene moves: some vector must be non-zero"


@pytest.mark.parametrize("h,w", SIZES + [(512, 768)])
def test_warp_is_exact(h, w):
    """Three channels and one, along vectors that are smooth (a real match) and along random vectors up to +-46 (every clamp at the
    borders, every fraction)."""
    _need_gpu()
    from ccedit_amd import ops
    src = scene(h, w, 3, 5)
    rs = np.random.RandomState(6)
    rows = [(0, 2, 1, 1), (1, 0, 0, 1)]
    vec = rs.randint(-46, 47, (2, h // 8, w // 8, 2)).astype(np.int32)
    vec[1] = ref.match(*[ref.pyramid(ref.luma(src[i])) for i in (1, 0)])
    edited = random_frames(h, w, 2, 7)
    luma = np.stack([ref.luma(f) for f in src])
    got3 = ops.prop_warp(_dev(edited), _dev(vec), _pairs(rows), 2).cpu().numpy()
    got1 = ops.prop_warp(_dev(luma), _dev(vec), _pairs(rows), 1).cpu().numpy()
    for i, (f, k, e, _) in enumerate(rows):
        fl = ref.flow(vec[i], h, w)
        assert np.array_equal(got3[i], ref.warp(edited[e], fl)), (h, w, i)
        assert np.array_equal(got1[i], ref.warp(luma[k], fl)), (h, w, i)
    const = np.broadcast_to(np.asarray([3, -2], np.int32), (1, h // 8, w // 8, 2)).copy()            # four equal vectors: exactly 16 v
    assert np.array_equal(ref.flow(const[0], h, w), np.broadcast_to(np.asarray([48, -32]), (h, w, 2)))
    shifted = ops.prop_warp(_dev(luma), _dev(const), _pairs([(0, 1, 0, 1)]), 1).cpu().numpy()[0]
    assert np.array_equal(shifted[0:h - 3, 2:w], luma[1][3:h, 0:w - 2])


@pytest.mark.parametrize("h,w", SIZES + [(512, 768)])
@pytest.mark.parametrize("masked", [False, True])
def test_blend_is_exact(h, w, masked):
    _need_gpu()
    from ccedit_amd import ops
    from ccedit_amd.propagate import device_tables
    rs = np.random.RandomState(8)
    nf, frames = 2, 3
    src = scene(h, w, frames, 9)
    w_rgb = random_frames(h, w, 2 * nf, 10)
    luma = np.stack([ref.luma(f) for f in src])
    # warped lumas: near the frame's own luma in places (high confidence), far in others, anything elsewhere
    w_luma = rs.randint(0, 256, (2 * nf, h, w)).astype(np.uint8)
    w_luma[0, :, : w // 2] = luma[1][:, : w // 2]
    w_luma[1, : h // 2] = np.clip(luma[1][: h // 2].astype(int) + rs.randint(-6, 7, (h // 2, w)), 0, 255)
    w_luma[2] = luma[2]
    rows = [(1, 0, 0, 5), (1, 2, 1, 2), (2, 0, 0, 1), (2, 1, 1, 255)]
    masks = rs.randint(0, 2, (frames, h, w)).astype(np.uint8) * rs.randint(128, 256, (frames, h, w)).astype(np.uint8) if masked else None
    pyr = ops.prop_pyramid(_dev(src))
    _, g = device_tables(pyr.device)
    got = ops.prop_blend(_dev(w_rgb), _dev(w_luma), pyr, _pairs(rows), g, frames, rgb=_dev(src) if masked else None,
                         mask=_dev(masks) if masked else None).cpu().numpy()
    for j in range(nf):
        f = rows[2 * j][0]
        ea, eb = ref.box_error(w_luma[2 * j], luma[f]), ref.box_error(w_luma[2 * j + 1], luma[f])
        want = ref.blend(w_rgb[2 * j], w_rgb[2 * j + 1], ea, eb, rows[2 * j][3], rows[2 * j + 1][3])
        if masked:
            want = np.where((masks[f] >= 128)[..., None], want, src[f])
        assert np.array_equal(got[j], want), (h, w, j, int((got[j] != want).sum()))


# ---- 2. a clip as a whole --------------------------------------------------------------------------
CLIPS = [
    # (h, w, key_index, kind)
    (64, 64, [0, 1, 2], "random"),                       # gap 1: nothing in between
    (64, 64, [0, 2], "random"),                          # gap 2, N = 2
    (64, 64, [1, 8], "scene"),                           # gap 7, N = 2, not starting at frame 0
    (128, 192, [0, 2, 4, 6, 8, 10], "scene"),            # six keyframes at gap 2
    (128, 192, [0, 7, 14], "scene"),                     # gap 7
    (64, 64, [0, 7, 14, 21, 28, 35], "random"),          # six keyframes at gap 7, random bytes
    (128, 192, [0, 2, 9, 10], "scene"),                  # mixed gaps 2, 7, 1
    (512, 768, [0, 2], "scene"),                         # one 512 x 768 frame: a pair
]


@pytest.mark.parametrize("h,w,keys,kind", CLIPS)
def test_propagate_clip_is_exact(h, w, keys, kind):
    _need_gpu()
    from ccedit_amd.propagate import propagate_clip
    n = keys[-1] + 2
    src = random_frames(h, w, n, 11) if kind == "random" else scene(h, w, n, 12)
    edited = np.stack([edit(src[k]) for k in keys]) if kind == "scene" else random_frames(h, w, len(keys), 13)
    got = propagate_clip(_dev(src), keys, _dev(edited)).cpu().numpy()
    want = ref.propagate_clip(src, keys, edited)
    assert got.shape == want.shape == (keys[-1] - keys[0] + 1, h, w, 3)
    for i in range(got.shape[0]):
        assert np.array_equal(got[i], want[i]), (keys, i, int((got[i] != want[i]).sum()))
    for j, k in enumerate(keys):
        assert np.array_equal(got[k - keys[0]], edited[j])


def test_propagate_clip_with_masks_is_exact():
    _need_gpu()
    from ccedit_amd.propagate import propagate_clip
    h, w, keys = 64, 128, [0, 3, 6]
    src = scene(h, w, 8, 14)
    edited = np.stack([edit(src[k]) for k in keys])
    masks = np.zeros((8, h, w), np.uint8)
    for f in range(8):
        masks[f, :, 8 * f:] = 255                                               # a different mask on every frame
    got = propagate_clip(_dev(src), keys, _dev(edited), masks=_dev(masks)).cpu().numpy()
    assert np.array_equal(got, ref.propagate_clip(src, keys, edited, masks=masks))
    for f in (1, 2, 4, 5):
        assert np.array_equal(got[f][:, : 8 * f], src[f][:, : 8 * f])


def test_result_does_not_depend_on_the_pair_chunking():
    _need_gpu()
    from ccedit_amd.propagate import propagate_clip
    h, w, keys = 64, 128, [0, 7, 14]
    src = scene(h, w, 15, 15)
    edited = np.stack([edit(src[k]) for k in keys])
    outs = [propagate_clip(_dev(src), keys, _dev(edited), pair_chunk=c).cpu().numpy() for c in (2, 6, 10, 64, 1024)]
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])
    for bad in (0, 3, -2):
        with pytest.raises(ValueError):
            propagate_clip(_dev(src), keys, _dev(edited), pair_chunk=bad)


# ---- 3. device tables are clamped, not followed; bad arguments are reported ------------------------
def test_out_of_range_tables_and_pairs_are_clamped():
    _need_gpu()
    from ccedit_amd import ops
    from ccedit_amd.propagate import device_tables, match_pairs, rank_table
    h, w, frames = 64, 128, 3
    src = scene(h, w, frames, 16)
    pyr = ops.prop_pyramid(_dev(src))
    ranks, g = device_tables(pyr.device)
    big = 2 ** 31 - 1
    # frame numbers far outside the clip act as the first / the last frame
    wild = _pairs([(-7, big, -big, 1), (big, -1, big, 1)])
    tame = _pairs([(0, frames - 1, 0, 1), (frames - 1, 0, frames - 1, 1)])
    v_wild, v_tame = match_pairs(pyr, wild, frames, h, w), match_pairs(pyr, tame, frames, h, w)
    assert np.array_equal(v_wild.cpu().numpy(), v_tame.cpu().numpy())
    assert np.array_equal(ops.prop_warp(_dev(src), v_tame, wild, 1).cpu().numpy(), ops.prop_warp(_dev(src), v_tame, tame, 1).cpu().numpy())
    assert np.array_equal(ops.prop_warp(_dev(src), v_tame, wild, 2).cpu().numpy(), ops.prop_warp(_dev(src), v_tame, tame, 2).cpu().numpy())
    # a rank table of garbage: vectors stay inside the search range of their level
    junk = _dev(np.asarray([big, -big] * 40 + [big], np.int32))
    v3 = ops.prop_match(pyr, tame, junk, None, frames, h, w, 3, 4).cpu().numpy()
    assert np.abs(v3).max() <= 4
    # parent vectors of garbage are held to +-32: the result equals that of the clamped parents
    nby, nbx = (h >> 3) // 8, (w >> 3) // 8
    par = np.random.RandomState(17).choice([-big, big, 1000, -33, 40, 0], size=(2, nby, nbx, 2)).astype(np.int32)
    got = ops.prop_match(pyr, tame, ranks[2], _dev(par), frames, h, w, 2, 2).cpu().numpy()
    want = ops.prop_match(pyr, tame, ranks[2], _dev(np.clip(par, -32, 32)), frames, h, w, 2, 2).cpu().numpy()
    assert np.array_equal(got, want) and np.abs(got).max() <= 66
    # block vectors of garbage in the warp: every sample stays inside the frame (held to +-4096, then the position is clamped)
    vec = np.random.RandomState(18).choice([-big, big, 5000, -5000], size=(2, h // 8, w // 8, 2)).astype(np.int32)
    got = ops.prop_warp(_dev(src), _dev(vec), tame, 1).cpu().numpy()
    want = ops.prop_warp(_dev(src), _dev(np.clip(vec, -4096, 4096)), tame, 1).cpu().numpy()
    assert np.array_equal(got, want)
    # the confidence table and the distances: entries outside 1 ... 4096 / 1 ... 255 are clamped
    w_rgb, w_luma = random_frames(h, w, 2, 19), random_frames(h, w, 2, 20)[..., 0].copy()
    gj = np.random.RandomState(21).choice([-big, big, 0, 5000, 7], size=256).astype(np.int32)
    got = ops.prop_blend(_dev(w_rgb), _dev(w_luma), pyr, _pairs([(1, 0, 0, -5), (1, 2, 1, 100000)]), _dev(gj), frames).cpu().numpy()
    want = ops.prop_blend(_dev(w_rgb), _dev(w_luma), pyr, _pairs([(1, 0, 0, 1), (1, 2, 1, 255)]), _dev(np.clip(gj, 1, 4096)), frames).cpu().numpy()
    assert np.array_equal(got, want)
    luma1 = ref.luma(src[1])
    ea, eb = ref.box_error(w_luma[0], luma1), ref.box_error(w_luma[1], luma1)
    assert np.array_equal(want[0], ref.blend(w_rgb[0], w_rgb[1], ea, eb, 1, 255, g=np.clip(gj, 1, 4096)))
    assert rank_table(4).max() == 80


def test_bad_arguments_are_reported():
    _need_gpu()
    from ccedit_amd import hip, ops
    from ccedit_amd.propagate import device_tables, propagate_clip
    src = _dev(random_frames(64, 64, 3, 22))
    pyr = ops.prop_pyramid(src)
    ranks, g = device_tables(src.device)
    pairs = _pairs([(1, 0, 0, 1), (1, 2, 1, 1)])
    with pytest.raises(ValueError):
        ops.prop_pyramid(src.cpu())
    with pytest.raises(ValueError):
        ops.prop_pyramid(src.float())
    with pytest.raises(hip.HipLibraryError, match="multiples of 64"):
        ops.prop_pyramid(_dev(random_frames(64, 96, 1, 23)))
    with pytest.raises(ValueError):
        ops.prop_match(pyr, pairs.long(), ranks[3], None, 3, 64, 64, 3, 4)
    with pytest.raises(ValueError):
        ops.prop_match(pyr, pairs, ranks[2], None, 3, 64, 64, 3, 4)              # a 25-entry table for radius 4
    out = torch.empty((2, 1, 1, 2), dtype=torch.int32, device=src.device)
    with pytest.raises(hip.HipLibraryError, match="level"):            # (a level beyond the pyramid: through the library itself)
        hip.check(hip.lib().ccedit_prop_match(pyr.data_ptr(), pairs.data_ptr(), ranks[3].data_ptr(), None, out.data_ptr(), 2, 3, 64, 64, 4, 4, None),
                  "ccedit_prop_match")
    vec = ops.prop_match(pyr, pairs, ranks[0], None, 3, 64, 64, 0, 2)
    with pytest.raises(ValueError):
        ops.prop_warp(src, vec[:, :4].contiguous(), pairs, 1)
    with pytest.raises(hip.HipLibraryError, match="col"):
        ops.prop_warp(src, vec, pairs, 3)
    w_rgb, w_luma = ops.prop_warp(src, vec, pairs, 1), ops.prop_warp(ops.prop_level(pyr, 3, 64, 64, 0), vec, pairs, 1)
    with pytest.raises(ValueError, match="together"):
        ops.prop_blend(w_rgb, w_luma, pyr, pairs, g, 3, rgb=src)
    with pytest.raises(ValueError):
        ops.prop_blend(w_rgb, w_luma, pyr, pairs, g[:100].contiguous(), 3)
    ed = _dev(random_frames(64, 64, 2, 24))
    with pytest.raises(ValueError, match="strictly increasing"):
        propagate_clip(src, [1, 1], ed)
    with pytest.raises(ValueError):
        propagate_clip(src, [0, 2], ed[:1])
    with pytest.raises(ValueError):
        propagate_clip(src.cpu(), [0, 2], ed)
    with pytest.raises(ValueError):
        propagate_clip(src, [0, 2], ed, masks=_dev(np.zeros((2, 64, 64), np.uint8)))


# ---- 4. the entry point, end to end ----------------------------------------------------------------
def _write_config(tmp_path):
    import yaml
    from ccedit_amd.sgm_compat import engine_config
    cfg = os.path.join(str(tmp_path), "tv2v.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump(dict(model=engine_config(crossframe=False, vae_ch=32, model_channels=64, num_heads=2, context_dim=64)), f)
    return cfg


def _gif_frames(path):
    from PIL import Image, ImageSequence
    return np.stack([np.array(fr.convert("RGB")) for fr in ImageSequence.Iterator(Image.open(path))])


@pytest.mark.timeout(1500)
def test_entry_point_writes_every_frame(tmp_path, monkeypatch):
    """sampling_tv2v.py --propagate on a frame directory of 18 frames, 6 keyframes at gap 3 (--synthetic): result_full/ holds frames
    0 ... 15, the keyframe positions are result/'s frames, log_info.json names the files; one run goes through --window_frames 3, the
    other through --inpainting_mode --mask_composite with a mask per frame: outside each frame's own mask the resized source frame.
    The uint8 frames are also caught on their way to the gif writer (a gif holds at most 256 colours per frame)."""
    _need_gpu()
    from PIL import Image
    from scripts.sampling import sampling_tv2v as S
    from scripts.sampling import util as U
    cfg = _write_config(tmp_path)
    rs = np.random.RandomState(6)
    vdir = tmp_path / "clips" / "fox"
    mdir = tmp_path / "clips" / "fox.mask"
    vdir.mkdir(parents=True)
    mdir.mkdir()
    big = _textured(90 + 40, 150 + 40, 30)
    masks = []
    for i in range(18):
        Image.fromarray(big[i:i + 90, 2 * i:2 * i + 150]).save(str(vdir / f"{i:03d}.png"))
        m = np.zeros((90, 150), np.uint8)
        m[:, 40 + 4 * i:] = 255                                                     # the kept region grows from frame to frame
        Image.fromarray(m).save(str(mdir / f"{i:03d}.png"))
        masks.append(np.array(Image.fromarray(m).resize((128, 64), Image.NEAREST)) >= 128)
    source = np.stack([np.array(Image.open(str(vdir / f"{i:03d}.png")).resize((128, 64), Image.BICUBIC)) for i in range(18)])
    caught = []
    real_save = U.save_gif_u8
    monkeypatch.setattr(U, "save_gif_u8", lambda path, frames, fps: (caught.append((np.array(frames), fps)), real_save(path, frames, fps))[1])
    base = ["sampling_tv2v.py", "--config_path", cfg, "--synthetic", "--H", "64", "--W", "128", "--num_keyframes", "6", "--sample_steps", "2",
            "--sampler_name", "DPMPP2SAncestralSampler", "--original_fps", "9", "--target_fps", "3", "--noise_seed", "1", "--prompt", "a red fox",
            "--video_path", str(vdir), "--batch_size", "1", "--save_type", "gif", "--propagate"]
    try:
        for tag, extra in (("windows", ["--window_frames", "3", "--gpu_io"]), ("masked", ["--inpainting_mode", "--mask_composite"])):
            out = str(tmp_path / tag)
            monkeypatch.setattr(sys, "argv", base + ["--save_path", out] + extra)
            caught.clear()
            S.main()
            log = json.load(open(os.path.join(out, "default", "log_info.json")))
            assert log["fullrate_paths"] == [os.path.join(out, "default", "result_full", "gif", "animation-0000.gif")], log
            assert len(log["keyframes_paths"]) == 1
            full, keys = _gif_frames(log["fullrate_paths"][0]), _gif_frames(log["keyframes_paths"][0])
            assert full.shape == (16, 64, 128, 3) and keys.shape == (6, 64, 128, 3), (full.shape, keys.shape)
            # --original_fps 9: 111 ms per frame asked of the writer; a gif stores the delay in hundredths of a second (11 -> 110 ms)
            assert Image.open(log["fullrate_paths"][0]).info["duration"] == int(round(1000.0 / 9)) // 10 * 10
            assert Image.open(log["keyframes_paths"][0]).info["duration"] == int(round(1000.0 / 3)) // 10 * 10
            assert np.array_equal(full[0::3], keys), f"{tag}: the frames at keyframe positions differ from result/"
            assert len(caught) == 1 and caught[0][1] == 9
            u8 = caught[0][0]
            assert u8.shape == (16, 64, 128, 3) and u8.dtype == np.uint8
            assert len({u8[f].tobytes() for f in range(16)}) == 16, "frames repeat"
            # the same call outside the entry point, from the frames the entry point used as keyframes
            from ccedit_amd.propagate import propagate_clip
            mk = _dev(np.stack(masks).astype(np.uint8) * 255) if extra[0] == "--inpainting_mode" else None
            again = propagate_clip(_dev(source), list(range(0, 18, 3)), _dev(u8[0::3]), masks=mk).cpu().numpy()
            assert np.array_equal(again, u8), tag
            if extra[0] == "--inpainting_mode":
                for f in (f for f in range(16) if f % 3):                        # (keyframe positions are result/'s frames, checked above)
                    keep = ~masks[f]
                    assert keep.any() and np.array_equal(u8[f][keep], source[f][keep]), f"frame {f}: kept pixels differ from the source frame"
                    assert (u8[f][~keep] != source[f][~keep]).mean() > 0.5, f"frame {f}: the edited region equals the source"
    finally:
        torch.set_grad_enabled(True)
    plain = S.parse_args(base[1:-1])
    assert plain.propagate is False
