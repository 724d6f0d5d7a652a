"""Automatic edit masks without a GPU (ccedit_amd/automask.py, --mask_auto): the rank rule, every refusal of the command line before a
video is opened, the properties of the numpy restatement the kernels are held to (tests/_automask_numpy.py) — a rectangle comes out as
the rectangle, specks and one-frame flicker go — the round trip through mask_latent's rule, and the table and files of --mask_auto_save."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _automask_numpy as AN  # noqa: E402

JOB = ["--prompt", "a zebra", "--video_path", "clips/horse"]
AUTO = ["--mask_auto", "--inpainting_mode", "--source_prompt", "a brown horse"] + JOB


def _args(*argv, ref=False):
    from scripts.sampling import sampling_tv2v as S
    from scripts.sampling import sampling_tv2v_ref as R
    return (R if ref else S).parse_args(list(argv))


# ---- 1. the rank ---------------------------------------------------------------------------------
def test_rank_of_edges():
    from ccedit_amd import automask
    for fn in (automask.rank_of, AN.rank_of):
        assert fn(0.0, 1920) == 1, "q = 0 is the minimum, rank 1"
        assert fn(1.0, 1920) == 1920 and fn(1.0, 1) == 1
        assert fn(0.0, 1) == 1 and fn(0.5, 1) == 1 and fn(0.99, 1) == 1
        for n in (1, 2, 3, 10, 384, 1920):
            assert fn(1.0 / n, n) == 1, n
        assert fn(0.99, 1920) == 1901 and fn(0.5, 1920) == 960 and fn(0.5, 5) == 3
    rs = np.random.RandomState(0)
    for q, n in zip(rs.rand(200), rs.randint(1, 200000, 200)):
        r = automask.rank_of(q, n)
        assert r == AN.rank_of(q, n) and 1 <= r <= n


# ---- 2. options and refusals ---------------------------------------------------------------------
def test_the_flags_parse_and_default():
    a = _args(*AUTO)
    assert a.mask_auto and a.source_prompt == "a brown horse"
    assert (a.mask_auto_samples, a.mask_auto_strength, a.mask_auto_quantile, a.mask_auto_threshold, a.mask_auto_vote) == (4, 0.5, 0.99, 0.5, 14)
    assert a.mask_auto_seed is None and a.mask_auto_save == ""
    from scripts.sampling import sampling_tv2v as S
    assert S.mask_auto_seed(a) == a.seed and S.mask_auto_seed(_args(*AUTO, "--mask_auto_seed", "7")) == 7
    plain = _args(*JOB)
    assert not S.mask_auto_on(plain)
    S.check_mask_auto(plain, with_ref=True)                        # without the flag nothing is refused anywhere


@pytest.mark.parametrize("argv,words", [
    (["--mask_auto", "--source_prompt", "x"] + JOB, "--inpainting_mode"),
    (["--mask_auto", "--inpainting_mode"] + JOB, "--source_prompt"),
    (["--mask_auto", "--inpainting_mode", "--source_prompt", "x"], "--video_path"),
    (AUTO + ["--mask_path", "m.png"], "--mask_path"),
    (AUTO + ["--mask_root", "masks"], "--mask_root"),
    (AUTO + ["--mask_track", "--H", "64", "--W", "128"], "--mask_track"),
    (AUTO + ["--propagate", "--mask_composite", "--save_type", "gif"], "--propagate --mask_composite"),
    (AUTO + ["--H", "68"], "multiples of 8"),
    (AUTO + ["--mask_auto_samples", "0"], "--mask_auto_samples"),
    (AUTO + ["--mask_auto_samples", "17"], "--mask_auto_samples"),
    (AUTO + ["--mask_auto_strength", "0"], "--mask_auto_strength"),
    (AUTO + ["--mask_auto_strength", "1.5"], "--mask_auto_strength"),
    (AUTO + ["--mask_auto_quantile", "1.01"], "--mask_auto_quantile"),
    (AUTO + ["--mask_auto_quantile", "-0.1"], "--mask_auto_quantile"),
    (AUTO + ["--mask_auto_threshold", "-1"], "--mask_auto_threshold"),
    (AUTO + ["--mask_auto_threshold", "nan"], "--mask_auto_threshold"),
    (AUTO + ["--mask_auto_vote", "28"], "--mask_auto_vote"),
    (AUTO + ["--mask_auto_vote", "-1"], "--mask_auto_vote"),
])
def test_refusals_name_their_flags(argv, words):
    with pytest.raises(ValueError) as e:
        _args(*argv)
    assert words in str(e.value) and "--mask_auto" in str(e.value), str(e.value)


def test_region_prompts_are_refused(tmp_path):
    from PIL import Image
    m = str(tmp_path / "m.png")
    Image.fromarray(np.zeros((64, 64), np.uint8)).save(m)
    with pytest.raises(ValueError, match="--region_prompt"):
        _args(*AUTO, "--region_prompt", "a snow field", "--region_mask", m)


def test_the_reference_image_script_refuses():
    from scripts.sampling import sampling_tv2v as S
    a = _args(*AUTO, "--reference_path", "r.png", ref=True)      # (its parser knows the flags: the refusal is main's, as for tiles)
    with pytest.raises(ValueError, match="sampling_tv2v_ref.py"):
        S.check_mask_auto(a, with_ref=True)


def test_boundary_options_pass():
    from ccedit_amd import automask
    automask.check_options(1, 1.0, 0.0, 0.0, 0)
    automask.check_options(16, 1e-3, 1.0, 10.0, 27)
    _args(*AUTO, "--mask_auto_vote", "0", "--mask_auto_samples", "16", "--mask_auto_quantile", "1", "--mask_composite", "--mask_dilate", "3",
          "--mask_invert")


# ---- 3. the restatement --------------------------------------------------------------------------
T, LH, LW = 5, 16, 24
RECT = (slice(4, 10), slice(6, 16))                                # 60 of 384 cells per frame: 15.6 %


def _rectangle_halves(seed, b=1, c=4):
    """Two halves that differ by 1.0 per channel inside RECT and by at most 0.1 per channel outside."""
    rs = np.random.RandomState(seed)
    src = rs.standard_normal((b, c, T, LH, LW)).astype(np.float32)
    delta = (rs.uniform(-0.1, 0.1, src.shape)).astype(np.float32)
    delta[:, :, :, RECT[0], RECT[1]] = np.where(rs.rand(b, c, T, 6, 10) < 0.5, -1.0, 1.0)
    inside = np.zeros((b, T, LH, LW), bool)
    inside[:, :, RECT[0], RECT[1]] = True
    assert inside.mean() >= 0.05
    return np.concatenate([src, (src + delta).astype(np.float32)]), inside


def test_accumulate_order_and_sign():
    y, _ = _rectangle_halves(1, b=2)
    acc = AN.accumulate(y)
    assert acc.dtype == np.float32 and acc.shape == (2, T, LH, LW) and (acc >= 0).all()
    d = [np.abs(y[2:, c] - y[:2, c]) for c in range(4)]
    assert np.array_equal(acc, ((d[0] + d[1]) + d[2]) + d[3])
    assert np.array_equal(AN.accumulate(y, acc), acc + acc)
    assert np.array_equal(AN.accumulate(y[[2, 3, 0, 1]]), acc), "the difference is symmetric in the halves"
    z = np.zeros((2, 1, 1, 1, 2), np.float32)
    z[0, 0, 0, 0, 0] = -0.0
    z[1, 0, 0, 0, 1] = -0.0
    assert np.array_equal(AN.accumulate(z).view(np.int32), np.zeros((1, 1, 1, 2), np.int32)), "signed zeros give +0"
    z[1, 0, 0, 0, 0] = np.nan
    assert np.isnan(AN.accumulate(z)[0, 0, 0, 0]) and AN.accumulate(z)[0, 0, 0, 1] == 0


@pytest.mark.parametrize("samples", [1, 3])
def test_a_rectangle_comes_out_as_the_rectangle(samples):
    acc, inside = None, None
    for k in range(samples):
        y, inside = _rectangle_halves(10 + k)
        acc = AN.accumulate(y, acc)
    assert acc[inside].min() > 3.9 * samples and acc[~inside].max() <= 0.4 * samples + 1e-5
    plain = AN.vote(AN.binarize(acc, 0.99, 0.5), 0)
    assert np.array_equal(plain.astype(bool), inside), "V = 0: the rectangle exactly"
    want = inside.copy()
    for cy in (4, 9):
        for cx in (6, 15):
            want[:, :, cy, cx] = False                             # a corner has 4 of 9 cells per frame: 12 of 27
    got = AN.vote(AN.binarize(acc, 0.99, 0.5), 14)
    assert np.array_equal(got.astype(bool), want), "V = 14: the rectangle minus its four corner cells in every frame"
    px = AN.mask_from(acc, 0.99, 0.5, 14)
    assert px.shape == (1, T, 8 * LH, 8 * LW) and px.dtype == np.uint8 and set(np.unique(px)) == {0, 255}
    assert np.array_equal(AN.mask_latent(px), got)


def test_binarize_is_strict_and_per_clip():
    acc = np.zeros((2, 1, 2, 4), np.float32)
    acc[0] = np.arange(8, dtype=np.float32).reshape(1, 2, 4) * 0.25           # q = 1: scale 1.75
    acc[1] = np.arange(8, dtype=np.float32).reshape(1, 2, 4) * 2.0            # scale 14
    m = AN.binarize(acc, 1.0, 0.5)                                            # thresholds 0.875 and 7.0: a clip has its own
    assert m[0].reshape(-1).tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    assert m[1].reshape(-1).tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    acc[0] = np.arange(8, dtype=np.float32).reshape(1, 2, 4) * 0.5
    acc[0, 0, 0, 0] = 4.0                                                     # scale 4.0: threshold 2.0 == the cell holding 2.0
    m = AN.binarize(acc, 1.0, 0.5)
    assert m[0].reshape(-1).tolist() == [1, 0, 0, 0, 0, 1, 1, 1], "a cell equal to the threshold stays clear"
    assert AN.binarize(np.zeros((1, 1, 2, 2), np.float32), 0.99, 0.5).sum() == 0, "scale 0: nothing exceeds 0"


def test_specks_and_one_frame_flicker_go():
    m = np.zeros((1, T, LH, LW), np.uint8)
    m[0, :, 3:9, 5:12] = 1                                          # a steady block: stays, minus its corners
    m[0, 2, 13, 20] = 1                                             # one isolated cell
    m[0, 3, 11:15, 1:5] = 1                                         # a 4 x 4 block in ONE frame: at most 9 of 27
    out = AN.vote(m, 14)
    assert out[0, :, 13, 20].sum() == 0 and out[0, :, 11:15, 1:5].sum() == 0
    assert out[0, :, 4:8, 6:11].all() and out.sum() == T * (6 * 7 - 4)
    hole = np.ones((1, T, LH, LW), np.uint8)
    hole[0, 2, 8, 8] = 0                                            # and a one-cell, one-frame hole is filled
    assert AN.vote(hole, 14).all()
    assert np.array_equal(AN.vote(m, 0), m)
    assert AN.vote(m, 27).sum() <= AN.vote(m, 14).sum() <= AN.vote(m, 1).sum()
    assert np.array_equal(AN.vote(m, 1) >= m, np.ones(m.shape, bool)) and np.array_equal(AN.vote(m, 27) <= m, np.ones(m.shape, bool))


def test_vote_clamps_at_the_borders():
    full = np.ones((2, 1, 1, 1), np.uint8)
    assert AN.vote(full, 27).all(), "a 1 x 1 x 1 clip is its own 27 neighbours"
    m = np.zeros((1, 2, 3, 5), np.uint8)
    m[0, 0, 0, 0] = 1                                               # a corner counts itself 8 times: (t, y, x) each clamp once
    assert AN.vote(m, 8)[0, 0, 0, 0] == 1 and AN.vote(m, 9)[0, 0, 0, 0] == 0


@pytest.mark.parametrize("h,w", [(9, 13), (16, 24), (1, 1)])
def test_expand_round_trip(h, w):
    m = (np.random.RandomState(h).rand(2, 3, h, w) < 0.4).astype(np.uint8)
    px = AN.expand(m)
    assert px.shape == (2, 3, 8 * h, 8 * w) and set(np.unique(px)) <= {0, 255}
    assert np.array_equal(AN.mask_latent(px), m)
    assert np.array_equal(px[:, :, ::8, ::8], m * 255) and np.array_equal(px[:, :, 7::8, 7::8], m * 255)


# ---- 4. --mask_auto_save -------------------------------------------------------------------------
def test_nearest_keyframe_table():
    from ccedit_amd.automask import nearest_keyframe
    assert nearest_keyframe([0, 3, 6], 9) == [0, 0, 1, 1, 1, 2, 2, 2, 2]
    assert nearest_keyframe([0, 4], 6) == [0, 0, 0, 1, 1, 1], "frame 2 is as far from 0 as from 4: the earlier keyframe"
    assert nearest_keyframe([2, 4], 7) == [0, 0, 0, 0, 1, 1, 1], "frame 3 ties, frames before the first keyframe take it"
    assert nearest_keyframe([5], 3) == [0, 0, 0]
    with pytest.raises(ValueError):
        nearest_keyframe([], 3)


def test_saved_masks_are_what_mask_root_reads_back(tmp_path):
    from PIL import Image
    from scripts.sampling import sampling_tv2v as S
    from scripts.sampling.util import load_video_mask
    vdir = tmp_path / "clips" / "bear"
    vdir.mkdir(parents=True)
    for i in range(9):
        Image.fromarray(np.zeros((64, 128, 3), np.uint8)).save(str(vdir / f"{i:03d}.png"))
    a = _args("--mask_auto", "--inpainting_mode", "--source_prompt", "a bear", "--prompt", "a panda", "--video_path", str(vdir), "--H", "64", "--W",
              "128", "--num_keyframes", "3", "--original_fps", "9", "--target_fps", "3", "--mask_auto_save", str(tmp_path / "D"))
    masks = torch.from_numpy(AN.expand((np.random.RandomState(2).rand(1, 3, 8, 16) < 0.5).astype(np.uint8))[0])
    out = S.save_auto_masks(a, str(vdir), masks)
    assert out == str(tmp_path / "D" / "bear") and sorted(os.listdir(out)) == [f"{f:05d}.png" for f in range(9)]
    for f, k in enumerate([0, 0, 1, 1, 1, 2, 2, 2, 2]):
        assert np.array_equal(np.array(Image.open(os.path.join(out, f"{f:05d}.png"))), masks[k].numpy()), f
    b = _args("--inpainting_mode", "--prompt", "a panda", "--video_path", str(vdir), "--mask_root", str(tmp_path / "D"))
    assert S.find_mask(b, str(vdir)) == out
    back = load_video_mask(out, 9, 3, 3, (64, 128), 9)
    assert torch.equal(back, masks)
