"""JPEG sources decoded on a real MI355X (ccedit_amd/jpegdec.py, csrc/jpegdec.hip).

Exact (no tolerance anywhere): jpegdec.decode and the entropy stage alone against the numpy restatement (tests/_jpegdec_numpy.py, which
tests/test_jpegdec.py holds to Pillow byte for byte) over the grid of tests/_jpegdec_cases.py and the own encoder's streams; grouping
of mixed lists, independence of the frames-per-launch bound, the round trip through the GPU encoder; the entry level (frame
directory, .avi) against the Pillow route, which is obtained by making the parser refuse; one sampling_tv2v.py job both ways.
LAST: twelve fixed corrupted streams, which must stop with the statuses the CPU gave and raise the error naming frame and interval."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _jpegdec_cases as K  # noqa: E402
import _jpegdec_numpy as R  # noqa: E402
import _mjpeg_numpy as E  # noqa: E402

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _by_size():
    """The grid + the own encoder's streams, as one list of names per frame size (decode returns one tensor per size)."""
    ref = K.reference()
    sizes = {}
    for name, _ in K.grid() + K.own_encoder():
        sizes.setdefault((ref[name][0].height, ref[name][0].width), []).append(name)
    return sizes


# ---- 1. bit equality -------------------------------------------------------------------------------
def test_decode_equals_the_restatement_over_the_grid():
    """Every size's streams in ONE call: all subsamplings, qualities, Huffman tables, restart layouts and contents of that size, so
    the call is also a list of mixed geometries and tables that has to be grouped and put back in order."""
    _need_gpu()
    from ccedit_amd import jpegdec
    ref, jp = K.reference(), dict(K.grid() + K.own_encoder())
    seen = 0
    for (h, w), names in _by_size().items():
        got = jpegdec.decode([jp[n] for n in names], "cuda").cpu().numpy()
        assert got.shape == (len(names), h, w, 3) and got.dtype == np.uint8
        differ = [n for i, n in enumerate(names) if not np.array_equal(got[i], ref[n][3])]
        assert not differ, f"{h}x{w}: {len(differ)} of {len(names)} frames differ from the restatement, first {differ[:5]}"
        seen += len(names)
    assert seen == 1792 + 8


def test_coefficients_equal_after_the_entropy_stage():
    _need_gpu()
    from ccedit_amd import jpegdec
    ref, jp = K.reference(), dict(K.grid() + K.own_encoder())
    for (h, w), names in _by_size().items():
        got = jpegdec.decode_coefficients([jp[n] for n in names], "cuda")
        for n, (coef, status) in zip(names, got):
            assert coef.dtype == np.int16 and np.array_equal(coef, ref[n][1]), n
            assert status.shape == ref[n][2].shape and not status.any(), n


def test_mixed_lists_are_grouped(monkeypatch):
    """Interleaved geometries and tables, repeated and in a scrambled order: each frame comes back at its own index."""
    _need_gpu()
    from ccedit_amd import jpegdec
    ref, jp = K.reference(), dict(K.grid())
    names = [n for n in _by_size()[(33, 50)] if "-q75-" in n or "-q100-" in n]
    order = np.random.default_rng(3).permutation(np.arange(2 * len(names))) % len(names)
    picked = [names[i] for i in order]
    keys = {ref[n][0].key() for n in picked}
    assert len(keys) > 20 and len(picked) > len(keys)
    launches = []
    real = jpegdec._entropy
    monkeypatch.setattr(jpegdec, "_entropy", lambda infos, jpegs, idx, device: (launches.append(list(idx)), real(infos, jpegs, idx, device))[1])
    got = jpegdec.decode([jp[n] for n in picked], "cuda").cpu().numpy()
    assert len(launches) == len(keys) and sorted(i for l in launches for i in l) == list(range(len(picked)))
    for l in launches:
        assert len({ref[picked[i]][0].key() for i in l}) == 1
    for i, n in enumerate(picked):
        assert np.array_equal(got[i], ref[n][3]), (i, n)
    with pytest.raises(ValueError, match="different sizes"):
        jpegdec.decode([jp[names[0]], jp[_by_size()[(48, 32)][0]]], "cuda")


def test_result_does_not_depend_on_the_frames_per_launch(monkeypatch):
    _need_gpu()
    from ccedit_amd import jpegdec
    ref, jp = K.reference(), dict(K.grid())
    names = [n for n in _by_size()[(17, 19)] if "-4:2:0-q95-std-rst-" in n] * 3 + [n for n in _by_size()[(17, 19)] if "-grey-q30-opt-norst-" in n] * 2
    assert len(names) == 20
    want = np.stack([ref[n][3] for n in names])
    outs = []
    for bound in (1, 3, len(names)):
        monkeypatch.setattr(jpegdec, "MAX_FRAMES_PER_LAUNCH", bound)
        outs.append(jpegdec.decode([jp[n] for n in names], "cuda").cpu().numpy())
    monkeypatch.setattr(jpegdec, "MAX_FRAMES_PER_LAUNCH", 256)
    monkeypatch.setattr(jpegdec, "SCRATCH_BYTES", 1)                         # the scratch bound alone: one frame per launch
    outs.append(jpegdec.decode([jp[n] for n in names], "cuda").cpu().numpy())
    for o in outs:
        assert np.array_equal(o, want)


def test_round_trip_through_the_gpu_encoder():
    """20 frames of 48 x 32: mjpeg.encode_frames -> jpegdec.decode equals the restatement's decode of the restatement's encode."""
    _need_gpu()
    from ccedit_amd import jpegdec, mjpeg
    frames = np.stack([K.content(("noise", "ramp", "primaries", "flat")[i % 4], 48, 32, 40 + i) for i in range(20)])
    frames[4:] = np.roll(frames[4:], 3, axis=2)
    jpegs = mjpeg.encode_frames(torch.from_numpy(frames).cuda(), 85)
    restated = E.encode_frames(frames, 85)
    assert jpegs == restated
    got = jpegdec.decode(jpegs, "cuda").cpu().numpy()
    assert np.array_equal(got, np.stack([R.decode(j) for j in restated]))


def test_argument_validation():
    _need_gpu()
    from ccedit_amd import jpegdec, ops
    j = dict(K.grid())["16x16-4:2:0-q75-std-rst-ramp"]
    info = jpegdec.parse(j)
    data, ivs, tab = jpegdec.pack_group([info], [j])
    d, i, t = (torch.from_numpy(a).cuda() for a in (data, ivs, tab))
    coef, status = ops.jpegdec_entropy(d, i, t, 1, 16, 16, 3, 2, 2, info.restart_interval)
    assert tuple(coef.shape) == (1, 6, 64) and tuple(status.shape) == (1, 1)
    with pytest.raises(ValueError, match="intervals"):
        ops.jpegdec_entropy(d, i[:0], t, 1, 16, 16, 3, 2, 2, info.restart_interval)
    with pytest.raises(ValueError, match="tables"):
        ops.jpegdec_entropy(d, i, t[:-1], 1, 16, 16, 3, 2, 2, info.restart_interval)
    with pytest.raises(ValueError, match="data"):
        ops.jpegdec_entropy(d.cpu(), i, t, 1, 16, 16, 3, 2, 2, info.restart_interval)
    with pytest.raises(Exception, match="sampling"):
        ops.jpegdec_entropy(d, i, t, 1, 16, 16, 3, 1, 2, info.restart_interval)
    with pytest.raises(ValueError, match="coefficients"):
        ops.jpegdec_idct(coef[:, :5].contiguous(), t, 16, 16, 3, 2, 2)
    planes = ops.jpegdec_idct(coef, t, 16, 16, 3, 2, 2)
    with pytest.raises(ValueError, match="planes"):
        ops.jpegdec_rgb(planes[:, :-1].contiguous(), 16, 16, 3, 2, 2)
    with pytest.raises(jpegdec.JpegUnsupported):
        jpegdec.decode([j[:40]], "cuda")
    with pytest.raises(ValueError, match="no frames"):
        jpegdec.decode([], "cuda")


# ---- 2. the entry level ----------------------------------------------------------------------------
def _refuse(monkeypatch):
    from ccedit_amd import jpegdec

    def parse(data):
        raise jpegdec.JpegUnsupported("refused by the test")
    monkeypatch.setattr(jpegdec, "parse", parse)


def _sources(tmp_path):
    from PIL import Image
    from ccedit_amd import mjpeg
    vdir = tmp_path / "frames"
    vdir.mkdir()
    for i in range(5):
        Image.fromarray(K.content(("ramp", "noise")[i % 2], 33, 50, 60 + i)).save(str(vdir / f"{i:03d}.jpg"), quality=88, subsampling=(2, 1, 0)[i % 3])
    frames = np.stack([K.content(("ramp", "primaries", "noise")[i % 3], 48, 32, 70 + i) for i in range(5)])
    avi = mjpeg.write_avi(str(tmp_path / "clip.avi"), E.encode_frames(frames, 90), 6, 48, 32)
    return str(vdir), avi


def test_loaders_equal_the_pillow_route(tmp_path, monkeypatch, capfd):
    """load_video_frames_u8 and load_video_keyframes with a device, on a directory of five 33 x 50 .jpg files and on a 5-frame 48 x 32
    .avi: bit-equal to the Pillow route (the parser made to refuse), which says on stderr why it was taken."""
    _need_gpu()
    from ccedit_amd import jpegdec, ops
    from scripts.sampling import util as U
    calls = []
    real = ops.jpegdec_rgb
    monkeypatch.setattr(ops, "jpegdec_rgb", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    outs = {}
    for src in _sources(tmp_path):
        for size in ((24, 40), None):
            if size:
                outs[src, "frames", size] = U.load_video_frames_u8(src, size, "cuda").cpu()
            outs[src, "keys", size] = U.load_video_keyframes(src, 6, 3, 2, size, device="cuda").cpu()
        outs[src, "img"] = U.load_img(os.path.join(src, "001.jpg"), (24, 40), device="cuda").cpu() if os.path.isdir(src) else None
    assert len(calls) >= 7
    capfd.readouterr()
    n = len(calls)
    _refuse(monkeypatch)
    for src in _sources_again(tmp_path):
        for size in ((24, 40), None):
            if size:
                assert torch.equal(outs[src, "frames", size], U.load_video_frames_u8(src, size, "cuda").cpu()), (src, size)
            assert torch.equal(outs[src, "keys", size], U.load_video_keyframes(src, 6, 3, 2, size, device="cuda").cpu()), (src, size)
        if os.path.isdir(src):
            assert torch.equal(outs[src, "img"], U.load_img(os.path.join(src, "001.jpg"), (24, 40), device="cuda").cpu())
    assert len(calls) == n, "the forced Pillow route launched the decoder"
    err = capfd.readouterr().err
    assert "refused by the test" in err and "decoded by Pillow on the host" in err
    assert outs[_sources_again(tmp_path)[1], "frames", (24, 40)].shape == (5, 24, 40, 3)


def _sources_again(tmp_path):
    return str(tmp_path / "frames"), str(tmp_path / "clip.avi")


def _write_config(tmp_path):
    import yaml
    from ccedit_amd.sgm_compat import engine_config
    cfg = os.path.join(str(tmp_path), "tv2v.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump(dict(model=engine_config(crossframe=False, vae_ch=32, model_channels=64, num_heads=2, context_dim=64)), f)
    return cfg


@pytest.mark.timeout(900)
def test_entry_point_writes_the_same_files_both_ways(tmp_path, monkeypatch):
    """sampling_tv2v.py --synthetic --gpu_io --propagate on an .avi source (8 frames, 3 keyframes at gap 3, 64 x 128 output): the device
    decoder and the forced Pillow route write byte-identical files."""
    _need_gpu()
    from PIL import Image  # noqa: F401
    from ccedit_amd import mjpeg, ops
    from scripts.sampling import sampling_tv2v as S
    cfg = _write_config(tmp_path)
    big = np.kron(K.content("noise", 20, 30, 9), np.ones((8, 8, 1), np.uint8))
    big = (big.astype(np.int32) * 3 // 4 + K.content("ramp", 160, 240, 0) // 4).astype(np.uint8)
    jpegs = [K.pillow_jpeg(big[2 * i:2 * i + 96, 4 * i:4 * i + 160], "4:2:0", 90, False, True) for i in range(8)]
    avi = mjpeg.write_avi(str(tmp_path / "fox.avi"), jpegs, 9, 96, 160)
    base = ["sampling_tv2v.py", "--config_path", cfg, "--synthetic", "--H", "64", "--W", "128", "--num_keyframes", "3", "--sample_steps", "2",
            "--sampler_name", "DPMPP2SAncestralSampler", "--original_fps", "9", "--target_fps", "3", "--noise_seed", "1", "--prompt", "a red fox",
            "--video_path", avi, "--batch_size", "1", "--save_type", "mjpeg", "--gpu_io", "--propagate"]
    calls = []
    real = ops.jpegdec_rgb
    monkeypatch.setattr(ops, "jpegdec_rgb", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    files = {}
    try:
        for tag in ("device", "pillow"):
            if tag == "pillow":
                assert calls, "the device route did not decode on the device"
                calls.clear()
                _refuse(monkeypatch)
            out = str(tmp_path / tag)
            monkeypatch.setattr(sys, "argv", base + ["--save_path", out])
            S.main()
            log = json.load(open(os.path.join(out, "default", "log_info.json")))
            files[tag] = {os.path.relpath(p, out): open(p, "rb").read() for kind in ("keyframes_paths", "fullrate_paths") for p in log[kind]}
            for root, _, names in os.walk(out):
                for nm in names:
                    if nm.endswith((".avi", ".png", ".gif")):
                        files[tag][os.path.relpath(os.path.join(root, nm), out)] = open(os.path.join(root, nm), "rb").read()
    finally:
        torch.set_grad_enabled(True)
    assert not calls, "the forced Pillow route launched the decoder"
    assert len(files["device"]) >= 2 and files["device"].keys() == files["pillow"].keys()
    for k in files["device"]:
        assert files["device"][k] == files["pillow"][k], f"{k}: the device decoder and the Pillow route wrote different bytes"
    assert len(mjpeg.read_avi(os.path.join(str(tmp_path / "device"), "default", "result_full", "mjpeg", "animation-0000.avi"))[0]) == 7


# ---- 3. LAST: corrupt entropy-coded data ----------------------------------------------------------
def test_zz_twelve_corrupted_streams_stop_with_the_cpu_statuses():
    """Twelve FIXED corrupted files (tests/_jpegdec_cases.py: byte flips inside the entropy-coded data that leave the file's layout
    alone), all of which the decode core ran clean under the host's sanitizers (tests/test_jpegdec.py).  On the device every interval
    ends with the status the CPU gave, and decode raises the error that names frame and interval."""
    _need_gpu()
    from ccedit_amd import jpegdec
    cases = K.gpu_corrupt_files(12)
    assert len(cases) == 12
    good = dict(K.grid())["16x16-4:4:4-q75-std-norst-ramp"]
    for name, data, want in cases:
        (coef, status), = jpegdec.decode_coefficients([data], "cuda", check=False)
        assert np.array_equal(status, want), (name, status, want)
        info = jpegdec.parse(data)
        first = int(np.flatnonzero(want)[0])
        text = re.escape(jpegdec.STATUS_TEXT[int(want[first])])
        if (info.height, info.width) == (16, 16):
            with pytest.raises(ValueError, match=f"frame 1, restart interval {first}: {text}"):
                jpegdec.decode([good, data], "cuda")
        with pytest.raises(ValueError, match=f"frame 0, restart interval {first}: {text}") as e:
            jpegdec.decode([data], "cuda")
        assert not isinstance(e.value, jpegdec.JpegUnsupported)
