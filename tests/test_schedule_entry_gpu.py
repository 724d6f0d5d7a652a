"""`--prompt_at` / `--prompt_ease` through scripts/sampling/sampling_tv2v.py on a real MI355X: a tiny synthetic job (the size of the
region and prompt entry tests), the log entry, the plain path for a schedule of one text, one run each composed with windows, tiles,
inpainting (with and without SDEdit), SDEdit, the prior mix, --gpu_io and long weighted prompts, and the refusals, which come before
anything is written.  --propagate and the gif / mjpeg / png writers work on the decoded frames after sampling and are not run here."""
import glob
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _write_config(tmp_path):
    import yaml
    from ccedit_amd.sgm_compat import engine_config
    cfg = os.path.join(str(tmp_path), "tv2v.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump(dict(model=engine_config(crossframe=False, vae_ch=32, model_channels=64, num_heads=2, context_dim=64)), f)
    return cfg


@pytest.fixture()
def clip(tmp_path):
    """A 64 x 128 frame directory of 9 frames (3 keyframes at 9 -> 3 fps) and a half-frame mask image."""
    from PIL import Image
    rs = np.random.RandomState(8)
    vdir = tmp_path / "clips" / "meadow"
    vdir.mkdir(parents=True)
    for i in range(9):
        Image.fromarray(rs.randint(0, 256, (64, 128, 3)).astype(np.uint8)).save(str(vdir / f"{i:03d}.png"))
    half = np.zeros((64, 128), np.uint8)
    half[:, 64:] = 255
    Image.fromarray(half).save(str(tmp_path / "half.png"))
    base = ["--config_path", _write_config(tmp_path), "--synthetic", "--H", "64", "--W", "128", "--num_keyframes", "3", "--sample_steps", "2",
            "--sampler_name", "DPMPP2SAncestralSampler", "--original_fps", "9", "--target_fps", "3", "--noise_seed", "1",
            "--prompt", "a meadow in summer", "--video_path", str(vdir), "--batch_size", "1", "--save_type", "npy"]
    return tmp_path, base


def _job(monkeypatch, base, out, *extra):
    """The job through scripts.sampling.sampling_tv2v.main in this process -> (result file's bytes, frames, log_info)."""
    from scripts.sampling import sampling_tv2v as S
    monkeypatch.setattr(sys, "argv", ["sampling_tv2v.py", *base, "--save_path", out, *extra])
    S.main()
    files = sorted(glob.glob(os.path.join(out, "default", "result", "npy", "frames-*.npy")))
    assert len(files) == 1, files
    with open(os.path.join(out, "default", "log_info.json")) as f:
        return open(files[0], "rb").read(), np.load(files[0]), json.load(f)


WINTER = ("--prompt_at", "2:a meadow in winter")


@pytest.mark.timeout(900)
def test_a_schedule_is_logged_and_changes_the_frames(clip, monkeypatch):
    _need_gpu()
    tmp_path, base = clip
    _, res, log = _job(monkeypatch, base, str(tmp_path / "sched"), *WINTER)
    assert res.shape == (3, 64, 128, 3) and np.isfinite(res).all()
    assert log["prompt_schedule"] == dict(keyed=[0, 2], ease="linear", frames=[[0, 1, 0.0], [0, 1, 0.5], [1, 1, 0.0]])
    _, plain, plog = _job(monkeypatch, base, str(tmp_path / "plain"))
    assert "prompt_schedule" not in plog and not np.array_equal(res, plain), "the schedule changed nothing"
    _, step, slog = _job(monkeypatch, base, str(tmp_path / "step"), *WINTER, "--prompt_ease", "step")
    assert slog["prompt_schedule"]["frames"] == [[0, 1, 0.0], [0, 1, 1.0], [1, 1, 0.0]] and not np.array_equal(step, res)


@pytest.mark.timeout(900)
def test_a_schedule_of_one_text_writes_the_plain_bytes(clip, monkeypatch):
    _need_gpu()
    tmp_path, base = clip
    one, _, log = _job(monkeypatch, base, str(tmp_path / "one"), "--prompt_at", "1:a meadow in summer", "--prompt_at=-1:a meadow in summer")
    plain, _, _ = _job(monkeypatch, base, str(tmp_path / "plain"))
    assert log["prompt_schedule"] == dict(keyed=[0, 1, 2], ease="linear", frames=[[0, 0, 0.0]] * 3)
    assert one == plain


@pytest.mark.timeout(900)
@pytest.mark.parametrize("name, extra", [
    ("windows", ("--window_frames", "2", "--window_overlap", "1")),
    ("tiles", ("--tile_h", "64", "--tile_w", "64")),
    ("inpainting", ("--inpainting_mode", "--mask_path", "HALF")),
    ("inpainting_sdedit", ("--inpainting_mode", "--mask_path", "HALF", "--sdedit_denoise_strength", "0.7")),
    ("sdedit", ("--sdedit_denoise_strength", "0.7")),
    ("prior_mix", ("--prior_coefficient_x", "0.3")),
    ("gpu_io", ("--gpu_io",)),
    ("long_weighted", ("--prompt_chunks", "2", "--prompt_syntax", "weighted")),
])
def test_a_schedule_composes(clip, monkeypatch, name, extra):
    _need_gpu()
    tmp_path, base = clip
    extra = tuple(str(tmp_path / "half.png") if e == "HALF" else e for e in extra)
    _, res, log = _job(monkeypatch, base, str(tmp_path / "sched"), *WINTER, *extra)
    _, plain, _ = _job(monkeypatch, base, str(tmp_path / "plain"), *extra)
    assert res.shape == (3, 64, 128, 3) and np.isfinite(res).all()
    assert log["prompt_schedule"]["keyed"] == [0, 2] and not np.array_equal(res, plain), f"{name}: the schedule changed nothing"
    if name == "long_weighted":
        assert [p["context_rows"] for p in log["prompts"]] == [154, 154]               # both texts of the schedule, one length


@pytest.mark.timeout(900)
def test_refusals_write_nothing(clip, monkeypatch):
    _need_gpu()
    tmp_path, base = clip
    out = str(tmp_path / "refused")
    half = str(tmp_path / "half.png")
    for extra, error, message in (
            (("--prompt_at", "3:winter"), ValueError, r"index 3 is outside the clip's 3 keyframes"),
            (("--prompt_at", "1:winter", "--prompt_at", "1:night"), ValueError, r"keyframe 1 is keyed twice"),
            (("--prompt_at", "1: "), ValueError, r"the text is empty"),
            ((*WINTER, "--region_prompt", "a bear", "--region_mask", half), NotImplementedError, r"--prompt_at with --region_prompt"),
            ((*WINTER, "--mask_auto", "--inpainting_mode", "--source_prompt", "a meadow"), NotImplementedError, r"--prompt_at with --mask_auto"),
            ((*WINTER, "--num_samples", "2", "--batch_size", "2"), ValueError, r"--prompt_at with --batch_size 2 and 2 clips")):
        with pytest.raises(error, match=message):
            _job(monkeypatch, base, out, *extra)
        assert not os.path.exists(os.path.join(out, "default", "result")), extra
    from scripts.sampling import sampling_tv2v_ref as R
    monkeypatch.setattr(sys, "argv", ["sampling_tv2v_ref.py", *base, "--save_path", out, *WINTER])
    with pytest.raises(NotImplementedError, match=r"--prompt_at is not available with a reference image"):
        R.main()
