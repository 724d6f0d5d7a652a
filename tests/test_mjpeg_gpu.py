"""Motion-JPEG output on a real MI355X (ccedit_amd/mjpeg.py, csrc/mjpeg.hip, --save_type mjpeg).

Exact (no tolerance anywhere): encode_frames and every stage against the numpy restatement (tests/_mjpeg_numpy.py, whose own worth
tests/test_mjpeg.py checks) on the images, sizes and qualities of that file, one to three frames per call, and one 512 x 768 pair.
Also: nothing around the frames is read into the result, repeats are bit-equal, the result does not depend on how frames are grouped
into calls or launches, garbage in the device tables is held in range, and the entry point end to end (--synthetic, a small frame
directory): both I/O routes write the same file, every frame decodes and lies within JPEG error of what --save_type gif hands its writer."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mjpeg_numpy as ref  # noqa: E402
from _mjpeg_images import IMAGES, QUALITIES, image, pil_decode, smoothed  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(16, 16), (48, 32), (160, 16), (64, 96)]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _frames(name, h, w, n):
    return np.stack([image(name, h, w, seed=s) if s == 0 or name in ("smooth", "random", "halfflat") else np.roll(image(name, h, w), 5 * s, axis=1)
                     for s in range(n)])


_CACHE = {}


def _expected(name, h, w, n, q):
    key = (name, h, w, n, q)
    if key not in _CACHE:
        _CACHE[key] = ref.encode_frames(_frames(name, h, w, n), q)
    return _CACHE[key]


# ---- 1. bit equality -------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", IMAGES)
def test_encode_frames_equals_the_restatement(name, size):
    _need_gpu()
    from ccedit_amd.mjpeg import encode_frames
    h, w = size
    for n in (1, 3):
        frames = _frames(name, h, w, n)
        if n == 3 and name not in ("black", "white"):
            assert len({f.tobytes() for f in frames}) == 3
        for q in QUALITIES:
            got = encode_frames(_dev(frames), q)
            want = _expected(name, h, w, n, q)
            assert [len(g) for g in got] == [len(x) for x in want], (name, size, n, q)
            assert got == want, (name, size, n, q)


@pytest.fixture(scope="module")
def production_pair():
    frames = np.stack([smoothed(512, 768, 11), smoothed(512, 768, 12)])
    coef = ref.transform(frames, 90)
    segs = ref.interval_bytes(coef)
    from ccedit_amd.mjpeg import frame_header
    return frames, coef, segs, [ref.assemble(frame_header(512, 768, 90), s) for s in segs]


def test_production_size_pair(production_pair):
    _need_gpu()
    from ccedit_amd.mjpeg import encode_frames
    frames, _, _, want = production_pair
    got = encode_frames(_dev(frames), 90)
    assert got == want
    assert pil_decode(got[1]).size == (768, 512)


# ---- 2. the stages ---------------------------------------------------------------------------------
@pytest.mark.parametrize("q", QUALITIES)
def test_stage_outputs(q):
    _need_gpu()
    from ccedit_amd import mjpeg as M
    from ccedit_amd import ops
    h, w, n = 48, 80, 2                                       # five MCUs per row: a full strip of four and a partial one
    frames = np.stack([image("random", h, w, 3), image("smooth", h, w, 4)])
    tab = M.device_tables("cuda")
    coef = ops.mjpeg_transform(_dev(frames), tab, q)
    want = ref.transform(frames, q)
    assert coef.dtype == torch.int16 and tuple(coef.shape) == (n, 3, 5, 6, 64)
    assert np.array_equal(coef.cpu().numpy(), want)
    segments, seg_len = ops.mjpeg_entropy(coef, tab)
    want_segs = [s for f in ref.interval_bytes(want) for s in f]
    assert seg_len.cpu().tolist() == [len(s) for s in want_segs]
    seg_np = segments.cpu().numpy()
    for i, s in enumerate(want_segs):
        assert seg_np[i, :len(s)].tobytes() == s, i
    hdr = M.frame_header(h, w, q)
    seg_off, frame_bytes = ops.mjpeg_pack_scan(seg_len, n, h, w, len(hdr))
    sizes = [len(hdr) + sum(len(s) + 2 for s in want_segs[3 * f:3 * f + 3]) for f in range(n)]
    assert frame_bytes.cpu().tolist() == sizes
    offs, at = [], 0
    for f in range(n):
        at += len(hdr)
        for s in want_segs[3 * f:3 * f + 3]:
            offs.append(at)
            at += len(s) + 2
    assert seg_off.cpu().tolist() == offs


def test_production_size_stages(production_pair):
    _need_gpu()
    from ccedit_amd import mjpeg as M
    from ccedit_amd import ops
    frames, want_coef, want_segs, _ = production_pair
    tab = M.device_tables("cuda")
    coef = ops.mjpeg_transform(_dev(frames), tab, 90)
    assert np.array_equal(coef.cpu().numpy(), want_coef)
    _, seg_len = ops.mjpeg_entropy(coef, tab)
    assert seg_len.cpu().tolist() == [len(s) for f in want_segs for s in f]


def test_extreme_coefficients_fit_the_segment():
    """The entropy stage alone, fed coefficients no transform produces: every AC at +-1023 after the clamp (values beyond it included),
    DC swinging between the extremes.  Each block then costs the most bits a block can; the lengths still equal the restatement's and
    stay inside the segment's slot."""
    _need_gpu()
    from ccedit_amd import mjpeg as M
    from ccedit_amd import ops
    rs = np.random.RandomState(5)
    coef = rs.choice(np.array([-32768, -1023, -1024, 1023, 32767, 600, -513], np.int16), size=(1, 2, 12, 6, 64)).astype(np.int16)
    coef[..., 0] = rs.choice(np.array([-1024, 1016, 0], np.int16), size=coef.shape[:-1])
    tab = M.device_tables("cuda")
    segments, seg_len = ops.mjpeg_entropy(_dev(coef), tab)
    want = ref.interval_bytes(coef)[0]
    assert seg_len.cpu().tolist() == [len(s) for s in want]
    assert max(len(s) for s in want) <= segments.shape[1]
    seg_np = segments.cpu().numpy()
    for i, s in enumerate(want):
        assert seg_np[i, :len(s)].tobytes() == s


def test_device_tables_are_held_in_range():
    """A table of garbage gives garbage bytes, but no access outside a buffer: lengths stay inside the slots, the canary stays put."""
    _need_gpu()
    from ccedit_amd import mjpeg as M
    from ccedit_amd import ops
    rs = np.random.RandomState(9)
    frames = _dev(image("random", 32, 48, 1)[None])
    for trial in range(3):
        bad = _dev(rs.randint(-2 ** 31, 2 ** 31 - 1, size=M.TAB_SIZE, dtype=np.int64).astype(np.int32))
        coef = ops.mjpeg_transform(frames, bad, 50)
        segments, seg_len = ops.mjpeg_entropy(coef, bad)
        torch.cuda.synchronize()
        lens = seg_len.cpu().numpy()
        assert (lens >= 0).all() and (lens <= segments.shape[1]).all()
    good = M.encode_frames(frames, 50)
    assert good == ref.encode_frames(frames.cpu().numpy(), 50)


# ---- 3. robustness ---------------------------------------------------------------------------------
def test_nothing_around_the_frames_is_read_or_written():
    _need_gpu()
    from ccedit_amd import mjpeg as M
    from ccedit_amd import ops
    h, w, n, q = 48, 32, 2, 90
    frames = _frames("smooth", h, w, n)
    nbytes = frames.size
    plain = M.encode_frames(_dev(frames), q)
    for fill in (0xA5, 0x00):
        big = torch.full((nbytes + 8192,), fill, dtype=torch.uint8, device="cuda")
        big[4096:4096 + nbytes] = _dev(frames).reshape(-1)
        inside = big[4096:4096 + nbytes].view(n, h, w, 3)
        assert inside.data_ptr() % 16 == 0
        assert M.encode_frames(inside, q) == plain
        assert bool((big[:4096] == fill).all()) and bool((big[4096 + nbytes:] == fill).all())
    # the outputs of every stage inside canaries
    tab = M.device_tables("cuda")
    hdr = torch.frombuffer(bytearray(M.frame_header(h, w, q)), dtype=torch.uint8).cuda()
    coef = ops.mjpeg_transform(_dev(frames), tab, q)
    segments, seg_len = ops.mjpeg_entropy(coef, tab)
    seg_off, frame_bytes = ops.mjpeg_pack_scan(seg_len, n, h, w, hdr.numel())
    total = int(frame_bytes.sum())
    out = ops.mjpeg_pack(segments, seg_len, seg_off, hdr, n, h, w, total)
    assert out.cpu().numpy().tobytes() == b"".join(plain)
    lens = seg_len.cpu().tolist()
    canary = torch.full_like(segments, 0x5A)
    from ccedit_amd import hip
    hip.check(hip.lib().ccedit_mjpeg_entropy(coef.data_ptr(), tab.data_ptr(), canary.data_ptr(), seg_len.data_ptr(), n, h, w,
                                             torch.cuda.current_stream().cuda_stream), "ccedit_mjpeg_entropy")
    c = canary.cpu().numpy()
    for i, ln in enumerate(lens):
        assert (c[i, ln:] == 0x5A).all(), f"segment {i}: bytes written behind its length"


def test_repeats_and_grouping():
    _need_gpu()
    from ccedit_amd import mjpeg as M
    h, w, n, q = 64, 96, 3, 90
    frames = _dev(_frames("halfflat", h, w, n))
    first = M.encode_frames(frames, q)
    assert first == _expected("halfflat", h, w, n, q)
    for _ in range(10):
        assert M.encode_frames(frames, q) == first
    assert [M.encode_frames(frames[i:i + 1], q)[0] for i in range(n)] == first
    old = M.SCRATCH_BYTES
    try:
        M.SCRATCH_BYTES = 1                                   # one frame per launch
        assert M.encode_frames(frames, q) == first
    finally:
        M.SCRATCH_BYTES = old


def test_encode_frames_refuses_what_it_cannot_code():
    _need_gpu()
    from ccedit_amd import mjpeg as M
    ok = _dev(np.zeros((1, 16, 16, 3), np.uint8))
    with pytest.raises(ValueError, match="24x16"):
        M.encode_frames(_dev(np.zeros((1, 24, 16, 3), np.uint8)), 90)
    with pytest.raises(ValueError, match="quality"):
        M.encode_frames(ok, 0)
    with pytest.raises(ValueError):
        M.encode_frames(ok.cpu(), 90)
    with pytest.raises(ValueError):
        M.encode_frames(ok.float(), 90)


def test_save_numbers_files_and_both_routes_write_the_same_bytes(tmp_path):
    _need_gpu()
    from ccedit_amd import mjpeg as M
    from scripts.sampling.util import perform_save_locally_video
    g = torch.Generator().manual_seed(2)
    x = torch.rand(2, 3, 4, 32, 48, generator=g)
    host, dev = str(tmp_path / "host"), str(tmp_path / "dev")
    p0 = perform_save_locally_video(host, x, 5, "mjpeg", return_savepaths=True)
    p1 = perform_save_locally_video(host, x[:1], 5, "mjpeg", return_savepaths=True, save_grid=False, video_quality=40)
    assert p0 == [os.path.join(host, "mjpeg", f"animation-{i:04}.avi") for i in range(2)]
    assert p1 == [os.path.join(host, "mjpeg", "animation-0002.avi")]
    assert sorted(os.listdir(os.path.join(host, "grid"))) == ["grid-0000.png", "grid-0001.png"]
    p2 = perform_save_locally_video(dev, x.cuda(), 5, "mjpeg", return_savepaths=True, gpu_io=True)
    assert [open(p, "rb").read() for p in p2] == [open(p, "rb").read() for p in p0]
    p3 = perform_save_locally_video(dev, (x * 2 - 1).cuda(), 5, "mjpeg", return_savepaths=True, gpu_io=True, signed=True, save_grid=False)
    assert len(p3) == 2
    jpegs, fps, h, w = M.read_avi(p0[1])
    assert (len(jpegs), fps, h, w) == (4, 5, 32, 48)
    u8 = (255.0 * x[1].permute(1, 2, 3, 0).numpy()).astype(np.uint8)
    assert jpegs == ref.encode_frames(u8, 90)
    assert len(open(p1[0], "rb").read()) < len(open(p0[0], "rb").read())
    assert M.read_avi(p1[0])[0] == ref.encode_frames((255.0 * x[0].permute(1, 2, 3, 0).numpy()).astype(np.uint8), 40)


# ---- 4. the entry point, end to end ----------------------------------------------------------------
def _write_config(tmp_path):
    import yaml
    from ccedit_amd.sgm_compat import engine_config
    cfg = os.path.join(str(tmp_path), "tv2v.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump(dict(model=engine_config(crossframe=False, vae_ch=32, model_channels=64, num_heads=2, context_dim=64)), f)
    return cfg


@pytest.mark.timeout(1500)
def test_entry_point_writes_motion_jpeg(tmp_path, monkeypatch):
    """sampling_tv2v.py --save_type mjpeg --propagate on a frame directory of 18 frames, 6 keyframes at gap 3 (--synthetic), with and
    without --gpu_io: the .avi files of the two routes are byte-identical, every frame decodes, and the decoded frames lie within JPEG
    error of the uint8 frames the --save_type gif run hands its writer — the bound is the restatement's own error on those frames + 1.
    result_full/mjpeg/ holds last - first + 1 = 16 frames at --original_fps."""
    _need_gpu()
    from PIL import Image
    from ccedit_amd import mjpeg as M
    from scripts.sampling import sampling_tv2v as S
    from scripts.sampling import util as U
    cfg = _write_config(tmp_path)
    vdir = tmp_path / "clips" / "fox"
    vdir.mkdir(parents=True)
    big = smoothed(90 + 40, 150 + 40, 30)
    for i in range(18):
        Image.fromarray(big[i:i + 90, 2 * i:2 * i + 150]).save(str(vdir / f"{i:03d}.png"))
    base = ["sampling_tv2v.py", "--config_path", cfg, "--synthetic", "--H", "64", "--W", "128", "--num_keyframes", "6", "--sample_steps", "2",
            "--sampler_name", "DPMPP2SAncestralSampler", "--original_fps", "9", "--target_fps", "3", "--noise_seed", "1", "--prompt", "a red fox",
            "--video_path", str(vdir), "--batch_size", "1", "--propagate"]
    caught = []
    real_save = U.save_gif_u8
    monkeypatch.setattr(U, "save_gif_u8", lambda path, frames, fps: (caught.append(np.array(frames)), real_save(path, frames, fps))[1])
    logs = {}
    try:
        for tag, extra in (("host", ["--save_type", "mjpeg"]), ("device", ["--save_type", "mjpeg", "--gpu_io"]), ("gif", ["--save_type", "gif"])):
            out = str(tmp_path / tag)
            monkeypatch.setattr(sys, "argv", base + ["--save_path", out] + extra)
            S.main()
            logs[tag] = json.load(open(os.path.join(out, "default", "log_info.json")))
    finally:
        torch.set_grad_enabled(True)
    for tag in ("host", "device"):
        out = str(tmp_path / tag)
        assert logs[tag]["keyframes_paths"] == [os.path.join(out, "default", "result", "mjpeg", "animation-0000.avi")]
        assert logs[tag]["fullrate_paths"] == [os.path.join(out, "default", "result_full", "mjpeg", "animation-0000.avi")]
    for kind in ("keyframes_paths", "fullrate_paths"):
        assert open(logs["host"][kind][0], "rb").read() == open(logs["device"][kind][0], "rb").read(), f"{kind}: the two I/O routes differ"
    jpegs, fps, h, w = M.read_avi(logs["host"]["fullrate_paths"][0])
    assert (len(jpegs), fps, h, w) == (16, 9, 64, 128)
    keys, kfps, _, _ = M.read_avi(logs["host"]["keyframes_paths"][0])
    assert (len(keys), kfps) == (6, 3)
    assert len(caught) == 1 and caught[0].shape == (16, 64, 128, 3)
    u8 = caught[0]                                               # what the gif run handed its writer: the same frames, never palettised
    restated = ref.encode_frames(u8, 90)
    assert jpegs == restated, "the .avi holds other frames than the encoder gives for the gif run's uint8 frames"
    decoded = np.stack([np.array(pil_decode(j)) for j in jpegs])
    own = np.stack([np.array(pil_decode(j)) for j in restated])
    bound = int(np.abs(own.astype(int) - u8.astype(int)).max()) + 1
    err = int(np.abs(decoded.astype(int) - u8.astype(int)).max())
    print(f"max |decoded - uint8 frames| = {err}, bound = {bound}")
    assert err <= bound
    assert [pil_decode(k).size for k in keys] == [(128, 64)] * 6
    assert keys == jpegs[0::3], "the frames at keyframe positions differ from result/"
    # the written file is a source of the next run
    assert U.count_video_frames(logs["host"]["fullrate_paths"][0]) == 16
    kf = U.load_video_keyframes(logs["host"]["fullrate_paths"][0], 9, 3, 6, (64, 128), device=torch.device("cuda"))
    assert tuple(kf.shape) == (6, 3, 64, 128)
