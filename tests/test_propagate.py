"""Full-frame-rate output, the part that needs no GPU (ccedit_amd/propagate.py, --propagate, tests/_propagate_numpy.py).

plan and the two tables; the refusals of the entry points (they run before a model is built); the new exports; and the numpy
restatement's own properties — the conditions the GPU tests (tests/test_propagate_gpu.py: kernels bit-equal to the restatement)
rely on: a static scene gives the integer cross-fade, integer translations are tracked exactly in the interior, and a faster
translation is still better than the cross-fade on every in-between frame."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _propagate_numpy as ref  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ---- plan ------------------------------------------------------------------------------------------
def test_plan_uniform_gaps():
    from ccedit_amd.propagate import plan
    p = plan([0, 7, 14], 20)
    assert p.first == 0 and p.last == 14 and p.num_out == 15
    assert p.frames.tolist() == [1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13]
    assert p.pairs.dtype == np.int32 and p.pairs.shape == (24, 4)
    for j, f in enumerate(p.frames):
        n = 0 if f < 7 else 1
        a, b = 7 * n, 7 * n + 7
        assert p.pairs[2 * j].tolist() == [f, a, n, b - f] and p.pairs[2 * j + 1].tolist() == [f, b, n + 1, f - a]


def test_plan_production_clip_and_long_clip():
    from ccedit_amd.propagate import plan
    p = plan(range(0, 17 * 7, 7), 120)                     # 17 keyframes at gap 7: 113 frames, 96 in between, 192 pairs
    assert p.num_out == 113 and len(p.frames) == 96 and p.pairs.shape == (192, 4)
    p = plan(range(3, 41 * 2 + 3, 2), 100)                 # a long clip (--window_frames): 41 keyframes at gap 2, not starting at 0
    assert p.first == 3 and p.last == 83 and len(p.frames) == 40 and (p.pairs[:, 3] == 1).all()
    assert p.pairs[:, 2].max() == 40


def test_plan_two_keyframes_and_gap_one():
    from ccedit_amd.propagate import plan
    p = plan([2, 5], 6)
    assert p.frames.tolist() == [3, 4] and p.pairs.tolist() == [[3, 2, 0, 2], [3, 5, 1, 1], [4, 2, 0, 1], [4, 5, 1, 2]]
    p = plan([0, 1, 2], 3)
    assert len(p.frames) == 0 and p.pairs.shape == (0, 4) and p.num_out == 3


@pytest.mark.parametrize("idx,n", [([0, 0, 1], 5), ([0, 2, 2, 3], 5), ([3, 2], 5), ([0], 5), ([0, 5], 5), ([-1, 2], 5), ([0, 300], 400)])
def test_plan_refuses(idx, n):
    from ccedit_amd.propagate import plan
    with pytest.raises(ValueError):
        plan(idx, n)


def test_plan_refuses_the_linspace_fallback_of_a_short_video():
    from ccedit_amd.propagate import plan
    from scripts.sampling.util import keyframe_indices
    idx = keyframe_indices(5, 20, 3, 9)                    # 5 frames, 9 keyframes asked: linspace repeats frames
    with pytest.raises(ValueError, match="strictly increasing"):
        plan(idx, 5)


# ---- tables ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 2, 4])
def test_rank_table_is_a_sorted_permutation(radius):
    from ccedit_amd.propagate import rank_table
    tab = rank_table(radius)
    n = 2 * radius + 1
    assert tab.dtype == np.int32 and sorted(tab.tolist()) == list(range(n * n)) and tab.max() < 256
    by_rank = sorted(range(n * n), key=lambda c: tab[c])
    keys = [(abs(c // n - radius) + abs(c % n - radius), c // n - radius, c % n - radius) for c in by_rank]
    assert keys == sorted(keys) and keys[0] == (0, 0, 0)
    assert np.array_equal(tab, ref.rank_table(radius))


def test_g_table_is_monotone_and_positive():
    from ccedit_amd.propagate import g_table
    g = g_table()
    assert g.dtype == np.int32 and g.shape == (256,) and g[0] == 4096 and g.min() >= 1 and (np.diff(g) <= 0).all()
    assert g[6] == 2048                                    # e = sigma: half the weight
    assert np.array_equal(g, ref.g_table())


def test_constants_have_one_place():
    from ccedit_amd import propagate as P
    for name in ("LEVELS", "BLOCK", "APRON", "RADIUS_COARSEST", "RADIUS_FINER", "BOX", "G_SCALE", "G_SIGMA"):
        assert getattr(P, name) == getattr(ref, name), name
    assert P.PAIR_CHUNK % 2 == 0 and P.radius_of(3) == 4 and P.radius_of(0) == 2


# ---- entry points ----------------------------------------------------------------------------------
def test_flag_parses_and_is_off_by_default():
    from scripts.sampling import sampling_tv2v as S
    from scripts.sampling import sampling_tv2v_ref as R
    assert S.parse_args([]).propagate is False and R.parse_args([]).propagate is False
    a = S.parse_args(["--propagate", "--save_type", "gif", "--prompt", "a fox", "--video_path", "clips/fox"])
    assert a.propagate is True
    assert R.parse_args(["--propagate", "--save_type", "gif", "--prompt", "a fox", "--video_path", "clips/fox"]).propagate is True
    helps = {act.dest: act.help for act in S.make_parser()._actions}
    assert "(not in the reference script)" in helps["propagate"]


@pytest.mark.parametrize("argv,needle", [
    (["--propagate", "--save_type", "gif"], "--video_path"),                                                  # outside job mode
    (["--propagate", "--save_type", "gif", "--video_path", "clips/fox"], "--prompt"),                       # a video but no prompt: not job mode
    (["--propagate", "--prompt", "a fox", "--video_path", "clips/fox"], "--save_type gif"),                 # npy (the default)
    (["--propagate", "--save_type", "mp4", "--prompt", "a fox", "--video_path", "clips/fox"], "--save_type gif"),
])
def test_flag_refusals_name_the_fix(argv, needle, capsys):
    from scripts.sampling import sampling_tv2v as S
    with pytest.raises(SystemExit):
        S.parse_args(argv)
    assert needle in capsys.readouterr().err


def test_short_video_is_refused_before_a_model_is_built(tmp_path, monkeypatch):
    from PIL import Image
    from scripts.sampling import sampling_tv2v as S
    vdir = tmp_path / "fox"
    vdir.mkdir()
    for i in range(5):
        Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(str(vdir / f"{i:03d}.png"))
    monkeypatch.setattr(S, "build_model", lambda *a, **k: pytest.fail("a model was built"))
    args = S.parse_args(["--propagate", "--save_type", "gif", "--prompt", "a fox", "--video_path", str(vdir), "--num_keyframes", "9",
                         "--save_path", str(tmp_path / "out")])
    with pytest.raises(ValueError, match="lower --num_keyframes"):
        S.run_jobs(args)
    S.check_propagate(S.parse_args(["--propagate", "--save_type", "gif", "--prompt", "a fox", "--video_path", str(vdir), "--num_keyframes", "2",
                                    "--original_fps", "4", "--target_fps", "1"]), [str(vdir)])                 # indices 0, 4: fine


def test_mask_loader_returns_all_frames(tmp_path):
    from PIL import Image
    from scripts.sampling.util import load_video_mask
    mdir = tmp_path / "m"
    mdir.mkdir()
    for i in range(7):
        m = np.zeros((8, 12), np.uint8)
        m[:, i:] = 255
        Image.fromarray(m).save(str(mdir / f"{i:03d}.png"))
    keys = load_video_mask(str(mdir), 3, 1, 3, None, 7)
    full = load_video_mask(str(mdir), 3, 1, 3, None, 7, all_frames=True)
    assert keys.shape == (3, 8, 12) and full.shape == (7, 8, 12) and np.array_equal(full[[0, 3, 6]].numpy(), keys.numpy())
    assert [int((full[i, 0] == 0).sum()) for i in range(7)] == list(range(7))
    Image.fromarray(np.full((8, 12), 255, np.uint8)).save(str(tmp_path / "one.png"))
    assert load_video_mask(str(tmp_path / "one.png"), 3, 1, 3, (16, 24), 7, all_frames=True).shape == (7, 16, 24)
    with pytest.raises(ValueError):
        load_video_mask(str(tmp_path / "one.png"), 3, 1, 3, None, None, all_frames=True)
    with pytest.raises(ValueError):
        load_video_mask(str(mdir), 3, 1, 3, None, 8, all_frames=True)


# ---- exports ---------------------------------------------------------------------------------------
def test_new_exports_are_declared_and_bound():
    from ccedit_amd import hip, ops
    src = open(os.path.join(ROOT, "include", "ccedit_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("ccedit_prop_pyramid", "ccedit_prop_match", "ccedit_prop_warp", "ccedit_prop_blend"):
        assert re.search(r"\b" + name + r"\s*\(", code), f"{name} is not declared in include/ccedit_hip.h"
        assert name in hip.EXPORTS
        assert hasattr(ops, name[len("ccedit_"):])
    assert hip.ABI_VERSION == 12 and "#define CCEDIT_ABI_VERSION 12" in src


def test_entry_points_report_bad_arguments():
    """Argument validation runs before any HIP call (as tests/test_cabi.py does for the other entry points)."""
    from ccedit_amd import hip
    lib = hip.lib()
    err = lambda: lib.ccedit_last_error()
    assert lib.ccedit_prop_pyramid(None, 16, 2, 64, 64, None) == -1 and b"null" in err()
    assert lib.ccedit_prop_pyramid(16, 16, 2, 64, 96, None) == -1 and b"multiples of 64" in err()
    assert lib.ccedit_prop_pyramid(18, 16, 2, 64, 64, None) == -1 and b"aligned" in err()
    assert lib.ccedit_prop_match(16, 16, 16, None, 16, 0, 2, 64, 64, 3, 4, None) == -1 and b"pairs" in err()
    assert lib.ccedit_prop_match(16, 16, 16, None, 16, 2, 2, 64, 64, 4, 4, None) == -1 and b"level" in err()
    assert lib.ccedit_prop_match(16, 16, 16, None, 16, 2, 2, 64, 64, 3, 5, None) == -1 and b"radius" in err()
    assert lib.ccedit_prop_match(16, 16, 16, 16, 16, 2, 2, 64, 64, 3, 4, None) == -1 and b"coarsest" in err()
    assert lib.ccedit_prop_match(16, 16, None, None, 16, 2, 2, 64, 64, 3, 4, None) == -1 and b"null" in err()
    assert lib.ccedit_prop_warp(16, 16, 16, 1, 16, 2, 2, 64, 64, 2, None) == -1 and b"channels" in err()
    assert lib.ccedit_prop_warp(16, 16, 16, 0, 16, 2, 2, 64, 64, 3, None) == -1 and b"col" in err()
    assert lib.ccedit_prop_warp(16, 16, 16, 1, 16, 2, 2, 100, 64, 3, None) == -1 and b"multiples of 64" in err()
    assert lib.ccedit_prop_blend(16, 16, 16, 16, 16, 16, None, 16, 1, 2, 64, 64, None) == -1 and b"together" in err()
    assert lib.ccedit_prop_blend(16, 16, 16, 16, 16, None, None, 16, 0, 2, 64, 64, None) == -1 and b"NF" in err()
    assert lib.ccedit_prop_blend(16, 16, 16, 16, None, None, None, 16, 1, 2, 64, 64, None) == -1 and b"null" in err()


# ---- the restatement's own properties --------------------------------------------------------------
def textured(h, w, seed, smooth=5):
    """Smoothed-noise RGB texture, full range."""
    rs = np.random.RandomState(seed)
    a = rs.randint(0, 256, (h, w, 3)).astype(np.float64)
    k = np.ones(smooth) / smooth
    for ax in (0, 1):
        a = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), ax, a)
    return ((a - a.min()) / (a.max() - a.min()) * 255).astype(np.uint8)


_LUT = np.random.RandomState(1).permutation(256).astype(np.uint8)


def edit(x):
    """The "edit" of the synthetic scenes: a per-pixel colour map, so the edit of any frame is known."""
    return np.stack([_LUT[x[..., 0]], 255 - x[..., 1], (x[..., 2] // 2 + _LUT[x[..., 1]] // 2).astype(np.uint8)], axis=-1)


def translating(h, w, dy, dx, frames, seed=0):
    big = textured(h + 200, w + 200, seed)
    return np.stack([big[100 + dy * t:100 + dy * t + h, 100 + dx * t:100 + dx * t + w] for t in range(frames)])


def test_static_scene_gives_the_integer_crossfade():
    src = translating(128, 192, 0, 0, 7)
    ed = np.stack([edit(src[0]), textured(128, 192, 5)])            # two DIFFERENT edited keyframes over a static source
    out = ref.propagate_clip(src, [0, 6], ed)
    assert np.array_equal(out[0], ed[0]) and np.array_equal(out[6], ed[1])
    for f in range(1, 6):
        a, b = ed[0].astype(np.int64), ed[1].astype(np.int64)
        assert np.array_equal(out[f], ((6 - f) * a + f * b + 3) // 6), f


def test_integer_translation_is_tracked_exactly_in_the_interior():
    src = translating(128, 192, 1, 2, 7)
    ed = np.stack([edit(src[0]), edit(src[6])])
    out = ref.propagate_clip(src, [0, 6], ed)
    for f in range(1, 6):
        assert np.array_equal(out[f][48:-48, 48:-48], edit(src[f])[48:-48, 48:-48]), f


def test_faster_translation_beats_the_crossfade_on_every_frame():
    src = translating(128, 192, 3, -5, 7)
    ed = np.stack([edit(src[0]), edit(src[6])])
    out = ref.propagate_clip(src, [0, 6], ed)
    for f in range(1, 6):
        truth = edit(src[f]).astype(np.int64)[48:-48, 48:-48]
        err = np.abs(out[f].astype(np.int64)[48:-48, 48:-48] - truth).mean()
        fade = np.abs(ref.crossfade(ed[0], ed[1], 6 - f, f).astype(np.int64)[48:-48, 48:-48] - truth).mean()
        print(f"frame {f}: propagated {err:.3f}, cross-fade {fade:.3f}, ratio {err / fade:.4f}")
        assert err < fade, (f, err, fade)


def test_masks_put_the_source_back_per_frame():
    src = translating(64, 64, 1, 1, 4)
    ed = np.stack([edit(src[0]), edit(src[3])])
    masks = np.zeros((4, 64, 64), np.uint8)
    masks[1, :, 32:] = 255
    masks[2, 32:, :] = 200
    out = ref.propagate_clip(src, [0, 3], ed, masks=masks)
    plain = ref.propagate_clip(src, [0, 3], ed)
    assert np.array_equal(out[1][:, :32], src[1][:, :32]) and np.array_equal(out[1][:, 32:], plain[1][:, 32:])
    assert np.array_equal(out[2][:32], src[2][:32]) and np.array_equal(out[2][32:], plain[2][32:])
    assert np.array_equal(out[0], ed[0]) and np.array_equal(out[3], ed[1])
