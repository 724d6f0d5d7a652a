"""GIF sources decoded on a real MI355X (ccedit_amd/gifdec.py, csrc/gifdec.hip).

Exact (no tolerance anywhere), over the served cases of tests/_gifdec_cases.py, stage by stage so that a failure points at one: the
stage A table against the reference's table (tests/_gifdec_numpy.py), the stage B indices against the reference's, the composited frames
against Pillow's.  Then `select`, independence of the launch grouping, the statuses of the stopped cases with their ValueError text, and
the loaders' opt-in route against the host route on clips from the project's two GIF writers."""
import functools
import io
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gifdec_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = sorted(K.all_served())


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@functools.lru_cache(maxsize=None)
def _stages(name):
    """Stages A and B of every frame of a file in ONE launch each -> (desc, table, ends, ncodes, status, planes), on the host."""
    from ccedit_amd import gifdec, ops
    info = K.expected(name)[0]
    data, desc, codes, plane, largest = gifdec.describe(info.frames, list(range(info.n_frames)))
    data_d, desc_d = torch.from_numpy(data).cuda(), torch.from_numpy(desc).cuda()
    table, ends, ncodes, status = ops.gifdec_codes(data_d, desc_d, codes)
    planes = ops.gifdec_pixels(desc_d, table, ends, ncodes, plane, largest)
    return desc, table.cpu().numpy(), ends.cpu().numpy(), ncodes.cpu().numpy(), status.cpu().numpy(), planes.cpu().numpy()


@pytest.mark.parametrize("name", NAMES)
def test_stage_a_the_code_table_equals_the_references(name):
    _need_gpu()
    from ccedit_amd import gifdec
    info, _, tables, _ = K.expected(name)
    desc, table, ends, ncodes, status, _ = _stages(name)
    assert np.array_equal(status, np.zeros_like(status)), status
    for i, (parent, length, first, last, off) in enumerate(tables):
        lo, n = int(desc[i, gifdec.D_CODE_OFF]), len(parent)
        assert ncodes[i] == n and n <= desc[i, gifdec.D_CODE_CAP], (i, ncodes[i], n)
        for got, want, what in ((table[0], parent, "parent"), (table[1], length, "len"), (table[2], off, "off"), (ends[0], first, "first"),
                                (ends[1], last, "last")):
            assert np.array_equal(got[lo:lo + n].astype(np.int64), want), (i, what)


@pytest.mark.parametrize("name", NAMES)
def test_stage_b_the_indices_equal_the_references(name):
    _need_gpu()
    from ccedit_amd import gifdec
    info, _, _, planes = K.expected(name)
    desc, _, _, _, _, got = _stages(name)
    for i, (f, want) in enumerate(zip(info.frames, planes)):
        lo = int(desc[i, gifdec.D_PLANE_OFF])
        assert np.array_equal(got[lo:lo + f.w * f.h], want), i


@pytest.mark.parametrize("name", NAMES)
def test_the_frames_equal_pillows(name):
    _need_gpu()
    from ccedit_amd import gifdec
    want = K.expected(name)[1]
    got = gifdec.decode_gif(K.all_served()[name], "cuda")
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want)


MULTI = ["rectangles-at-the-corners", "transparent-local-palette", "disposal-1", "short-palettes", "pillow-writer", "device-writer-format"]


@pytest.mark.parametrize("name", MULTI)
def test_select_and_the_launch_grouping_do_not_change_a_byte(name):
    """Frames picked out of order and twice; groups of 1 and of 2 frames (the canvas is carried between launches)."""
    _need_gpu()
    from ccedit_amd import gifdec
    data, want = K.all_served()[name], K.expected(name)[1]
    n = want.shape[0]
    for per in (1, 2, None):
        got = gifdec.decode_gif(data, "cuda", frames_per_group=per)
        assert np.array_equal(got.cpu().numpy(), want), per
    for pick in ([n - 1], [1], [n - 1, 0, n - 1], list(range(0, n, 2))):
        for per in (1, 2, None):
            got = gifdec.decode_gif(data, "cuda", select=lambda count: pick, frames_per_group=per)
            assert np.array_equal(got.cpu().numpy(), want[pick]), (pick, per)
    with pytest.raises(ValueError, match="frame indices"):
        gifdec.decode_gif(data, "cuda", select=lambda count: [count])


@pytest.mark.parametrize("name", sorted(K.stopped()))
def test_stopped_cases_return_their_status(name):
    _need_gpu()
    import _gifdec_numpy as R
    from ccedit_amd import gifdec
    data, status, frame = K.stopped()[name]
    info = gifdec.parse(data)
    f = info.frames[frame]
    where = R.code_table(f.stream, f.min_code, f.w * f.h)[6] if status != R.BAD_INDEX else None
    for per in (None, 1):
        with pytest.raises(ValueError) as e:
            gifdec.decode_gif(data, "cuda", frames_per_group=per)
        text = str(e.value)
        assert text.startswith(f"frame {frame}: {gifdec.STATUS_TEXT[status]} (code {status} at "), text
        if where is not None:
            assert text.endswith(f"at bit {where})"), text
        else:                                                          # the lowest offset in the plane of an index beyond the palette: all are
            assert text.endswith("at pixel 0)"), text
    first = gifdec.decode_gif(data, "cuda", select=lambda count: [0])                 # (the frames before the broken one are served)
    assert np.array_equal(first.cpu().numpy(), np.array(Image.open(io.BytesIO(data)).convert("RGB"))[None])


def test_the_loaders_opt_in_route_equals_the_host_route(tmp_path, capsys):
    _need_gpu()
    from scripts.sampling import util as U
    for name, data in K.writer_clips().items():
        path = str(tmp_path / f"{name}.gif")
        with open(path, "wb") as f:
            f.write(data)
        host = U.load_video_keyframes(path, 2, 1, 2)                                                      # frames 0 and 2, no resize
        dev = U.load_video_keyframes(path, 2, 1, 2, device="cuda", gif_decoder="device")
        assert torch.equal(dev.cpu(), host), name
        for size in (None, (32, 48)):
            pil = U.load_video_keyframes(path, 2, 1, 2, size, device="cuda")
            dev = U.load_video_keyframes(path, 2, 1, 2, size, device="cuda", gif_decoder="device")
            assert torch.equal(dev, pil), (name, size)
        assert torch.equal(U.load_video_frames_u8(path, (32, 48), "cuda", gif_decoder="device"), U.load_video_frames_u8(path, (32, 48), "cuda")), name
    assert capsys.readouterr().err == ""


def _write_config(tmp_path):
    import yaml
    from ccedit_amd.sgm_compat import engine_config
    cfg = os.path.join(str(tmp_path), "tv2v.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump(dict(model=engine_config(crossframe=False, vae_ch=32, model_channels=64, num_heads=2, context_dim=64)), f)
    return cfg


@pytest.mark.timeout(900)
def test_entry_point_writes_the_same_files_with_either_decoder(tmp_path, monkeypatch):
    """sampling_tv2v.py --synthetic --gpu_io --propagate --save_type gif on a .gif source (8 frames of 96 x 160 from Pillow's writer, 3
    keyframes at gap 3, 64 x 128 output): --gif_decoder device and the default write byte-identical files, and only the former decodes
    on the device."""
    _need_gpu()
    import json
    from _gif_cases import content
    from ccedit_amd import ops, video_io
    from scripts.sampling import sampling_tv2v as S
    cfg = _write_config(tmp_path)
    big = content("photo", 160, 240, 3)
    gif_path = video_io._write_gif_pillow(str(tmp_path / "fox.gif"), [big[2 * i:2 * i + 96, 4 * i:4 * i + 160] for i in range(8)], 9)
    base = ["sampling_tv2v.py", "--config_path", cfg, "--synthetic", "--H", "64", "--W", "128", "--num_keyframes", "3", "--sample_steps", "2",
            "--sampler_name", "DPMPP2SAncestralSampler", "--original_fps", "9", "--target_fps", "3", "--noise_seed", "1", "--prompt", "a red fox",
            "--video_path", gif_path, "--batch_size", "1", "--save_type", "gif", "--gpu_io", "--propagate"]
    calls = []
    real = ops.gifdec_codes
    monkeypatch.setattr(ops, "gifdec_codes", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    files = {}
    try:
        for tag, extra in (("device", ["--gif_decoder", "device"]), ("pillow", [])):
            if tag == "pillow":
                assert calls, "--gif_decoder device did not decode on the device"
                calls.clear()
            out = str(tmp_path / tag)
            monkeypatch.setattr(sys, "argv", base + extra + ["--save_path", out])
            S.main()
            log = json.load(open(os.path.join(out, "default", "log_info.json")))
            files[tag] = {os.path.relpath(p, out): open(p, "rb").read() for kind in ("keyframes_paths", "fullrate_paths") for p in log[kind]}
            for root, _, names in os.walk(out):
                for nm in names:
                    if nm.endswith((".png", ".gif")):
                        files[tag][os.path.relpath(os.path.join(root, nm), out)] = open(os.path.join(root, nm), "rb").read()
    finally:
        torch.set_grad_enabled(True)
    assert not calls, "the default route launched the GIF decoder"
    assert len(files["device"]) >= 2 and files["device"].keys() == files["pillow"].keys()
    for k in files["device"]:
        assert files["device"][k] == files["pillow"][k], f"{k}: the two decoders' runs wrote different bytes"
