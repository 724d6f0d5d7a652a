"""Long clips (ccedit_amd/windows.py, --window_frames): the host side — the window plan, the flags, what is refused.  No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _raw(j, t):
    return min(j + 1, t - j)


@pytest.mark.parametrize("t", [3, 4, 17])
def test_plan_covers_every_frame_with_normalised_weights(t):
    from ccedit_amd.windows import plan
    for overlap in range(t):
        step = t - overlap
        for n in range(t, 4 * t + 1):
            starts, coef = plan(n, t, overlap)
            assert starts[0] == 0 and starts[-1] == n - t, (n, t, overlap, starts)
            assert all(b > a for a, b in zip(starts, starts[1:])), (n, t, overlap, starts)
            assert all(b - a <= step for a, b in zip(starts, starts[1:])), (n, t, overlap, starts)
            assert isinstance(coef, np.ndarray) and coef.dtype == np.float32 and coef.shape == (len(starts), t)
            total = np.zeros(n, np.float64)
            cover = np.zeros(n, np.int64)
            for w, s in enumerate(starts):
                total[s:s + t] += coef[w].astype(np.float64)
                cover[s:s + t] += 1
            assert cover.min() >= 1, (n, t, overlap)
            assert np.abs(total - 1.0).max() < 1e-6, (n, t, overlap, np.abs(total - 1.0).max())
            for w, s in enumerate(starts):
                for j in range(t):
                    if cover[s + j] == 1:
                        assert coef[w, j] == np.float32(1.0), (n, t, overlap, w, j)
                    # the definition: r(j) / sum of r over the covering windows, from integers in float64, rounded once
                    d = sum(_raw(s + j - s2, t) for s2 in starts if 0 <= s + j - s2 < t)
                    assert coef[w, j] == np.float32(np.float64(_raw(j, t)) / np.float64(d)), (n, t, overlap, w, j)


def test_plan_known_cases():
    from ccedit_amd.windows import plan
    starts, coef = plan(17, 17, 8)
    assert starts == [0] and np.array_equal(coef, np.ones((1, 17), np.float32))
    assert plan(41, 17, 8)[0] == [0, 9, 18, 24]
    starts, coef = plan(6, 3, 1)
    assert starts == [0, 2, 3]
    # frames 0 1 | 2: windows 0 (r = 1) and 1 (r = 1) | 3: windows 1 (r = 2) and 2 (r = 1) | 4: windows 1 (r = 1) and 2 (r = 2) | 5
    want = np.array([[1, 1, 1 / 2], [1 / 2, 2 / 3, 1 / 3], [1 / 3, 2 / 3, 1]], np.float64).astype(np.float32)
    assert np.array_equal(coef, want)
    assert plan(34, 17, 0)[0] == [0, 17] and np.array_equal(plan(34, 17, 0)[1], np.ones((2, 17), np.float32))


@pytest.mark.parametrize("n,t,o", [(16, 17, 8), (17, 17, 17), (17, 17, -1), (17, 17, 18), (0, 3, 1), (5, 0, 0)])
def test_plan_refuses_bad_arguments(n, t, o):
    from ccedit_amd.windows import plan
    with pytest.raises(ValueError):
        plan(n, t, o)


def test_window_flags_parse_and_decide():
    from scripts.sampling import sampling_tv2v as S
    a = S.parse_args([])
    assert a.window_frames == 0 and a.window_overlap is None and not S.windowing(a)
    a = S.parse_args(["--window_frames", "17", "--num_keyframes", "41"])
    assert a.window_frames == 17 and a.window_overlap is None and S.windowing(a)
    a = S.parse_args(["--window_frames", "17", "--window_overlap", "4", "--num_keyframes", "41"])
    assert a.window_overlap == 4 and S.windowing(a)
    assert not S.windowing(S.parse_args(["--window_frames", "17", "--num_keyframes", "17"]))        # one window: the plain path
    assert not S.windowing(S.parse_args(["--window_frames", "17", "--num_keyframes", "9"]))
    helps = {act.dest: act.help for act in S.make_parser()._actions}
    assert "(not in the reference script)" in helps["window_frames"] and "(not in the reference script)" in helps["window_overlap"]
    for bad in (["--window_frames", "3", "--window_overlap", "3"], ["--window_overlap", "1"], ["--window_frames", "-2"]):
        with pytest.raises(SystemExit):
            S.parse_args(bad)


def test_default_overlap_is_half_a_window():
    from ccedit_amd.windows import WindowedDenoiser, plan
    w = WindowedDenoiser(lambda x, s, c: x, 17)
    assert w.overlap == 8
    assert WindowedDenoiser(lambda x, s, c: x, 3).overlap == 1
    with pytest.raises(ValueError):
        WindowedDenoiser(lambda x, s, c: x, 3, 3)
    assert plan(41, 17, w.overlap)[0] == [0, 9, 18, 24]


def _write_config(tmp_path, crossframe):
    import yaml
    from ccedit_amd.sgm_compat import engine_config
    cfg = os.path.join(str(tmp_path), "cfg.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump(dict(model=engine_config(crossframe=crossframe, vae_ch=32, model_channels=64, num_heads=2, context_dim=64)), f)
    return cfg


def test_windows_are_refused_under_the_ref_script(tmp_path, monkeypatch):
    """sampling_tv2v_ref.py --window_frames: NotImplementedError out of main(), before a model is built (no GPU here: building one
    would fail differently)."""
    from scripts.sampling import sampling_tv2v_ref as R
    cfg = _write_config(tmp_path, crossframe=True)
    argv = ["sampling_tv2v_ref.py", "--config_path", cfg, "--synthetic", "--window_frames", "3", "--num_keyframes", "6"]
    monkeypatch.setattr(sys, "argv", argv)
    with pytest.raises(NotImplementedError, match="window_frames"):
        R.main()
    monkeypatch.setattr(sys, "argv", argv + ["--prompt", "a fox", "--video_path", str(tmp_path)])          # job mode
    with pytest.raises(NotImplementedError, match="window_frames"):
        R.main()


def test_windows_are_refused_with_a_cond_feat_config(tmp_path, monkeypatch):
    from scripts.sampling import sampling_tv2v as S
    cfg = _write_config(tmp_path, crossframe=True)
    argv = ["sampling_tv2v.py", "--config_path", cfg, "--synthetic", "--window_frames", "3", "--num_keyframes", "6"]
    monkeypatch.setattr(sys, "argv", argv)
    with pytest.raises(NotImplementedError, match="cond_feat"):
        S.main()
    monkeypatch.setattr(sys, "argv", argv + ["--prompt", "a fox", "--video_path", str(tmp_path)])          # job mode
    with pytest.raises(NotImplementedError, match="cond_feat"):
        S.main()
    # the TV2V config passes the check; a clip that fits one window is never checked
    S.check_windowing(S.parse_args(["--config_path", _write_config(tmp_path, crossframe=False), "--window_frames", "3", "--num_keyframes", "6"]))
    S.check_windowing(S.parse_args(["--config_path", cfg, "--window_frames", "3", "--num_keyframes", "3"]))


def test_windows_are_refused_for_reference_conditioning_and_sharded_wrappers():
    import torch
    from ccedit_amd.windows import WindowedDenoiser, check_supported

    class Sharded:
        frame_shard, row_shard = object(), None

    class Rows:
        frame_shard, row_shard = None, object()

    for wr in (Sharded(), Rows()):
        with pytest.raises(NotImplementedError, match="sharded"):
            WindowedDenoiser(lambda x, s, c: x, 3, 1, wrapper=wr)
    with pytest.raises(NotImplementedError, match="cond_feat"):
        check_supported(cond=dict(crossattn=torch.zeros(1), control_hint=torch.zeros(1), cond_feat=torch.zeros(1)))
    check_supported(cond=dict(crossattn=torch.zeros(1), control_hint=torch.zeros(1)))
