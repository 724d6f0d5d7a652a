"""PNG / APNG output encoded on a real MI355X (ccedit_amd/png.py, csrc/png.hip, --save_type png).

Exact (no tolerance anywhere): every stage alone and encode_frames + write_apng against the numpy restatement (tests/_png_numpy.py, whose
own worth tests/test_png.py checks against zlib and Pillow) — the frame shapes and crafted byte streams of tests/_png_cases.py, crafted
tokens and histograms fed to the codes and emit stages directly, more frames than one launch takes, one full-size pair — and the entry
level: perform_save_locally_video with and without gpu_io, and one job of sampling_tv2v.py whose files Pillow decodes to the frames
--save_type npy holds."""
import json
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _png_cases as K  # noqa: E402
import _png_numpy as M  # noqa: E402
from ccedit_amd import png as P  # noqa: E402

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _words(a):
    """uint32 numpy words -> the int32 device tensor the ops take."""
    return _dev(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32))


def pillow_frames(path):
    im = Image.open(path)
    out = []
    for i in range(getattr(im, "n_frames", 1)):
        im.seek(i)
        out.append(np.array(im.convert("RGB")))
    return im, np.stack(out, axis=0)


def _mirror_file(tmp_path, frames, duration):
    return open(M.write_apng(str(tmp_path / "want.png"), frames, duration), "rb").read()


def _device_file(tmp_path, frames, duration):
    n, h, w, _ = frames.shape
    return open(P.write_apng(str(tmp_path / "got.png"), P.encode_frames(_dev(frames)), duration, w, h), "rb").read()


# ---- 1. the stages alone ---------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", K.SMALL_SHAPES + list(K.BORDER_SHAPES.values()))
def test_filter_stage(h, w):
    _need_gpu()
    from ccedit_amd import ops
    frames = K.clip(h, w, 5)
    got = ops.png_filter(_dev(frames))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (5, h, P.row_bytes(w))
    want = np.stack([M.filter_frame(f) for f in frames])
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("name", sorted(K.streams()))
def test_deflate_stages_on_crafted_streams(name):
    """tokens, codes, emit, pack and adler, each against the restatement's value for the same chunk, then the whole zlib stream."""
    _need_gpu()
    import zlib
    from ccedit_amd import ops
    data = K.streams()[name]
    chunks, stream = K.stream_reference(name)
    c = len(chunks)
    filtered = _dev(np.frombuffer(data, dtype=np.uint8).copy()[None])
    tokens, ntok, hist = ops.png_tokens(filtered)
    assert tuple(tokens.shape) == (c, P.CHUNK) and tuple(hist.shape) == (c, P.HIST_WORDS)
    assert ntok.cpu().tolist() == [len(t) for t, _, _, _ in chunks]
    for k, (tok, h, blk, bits) in enumerate(chunks):
        assert np.array_equal(_u32(tokens[k, :len(tok)]), tok), (name, k)
        assert np.array_equal(_u32(hist[k]), h), (name, k)
    codes, header, header_bits, chunk_bits = ops.png_codes(hist, 1)
    assert header_bits.cpu().tolist() == [blk.header.n for _, _, blk, _ in chunks]
    assert chunk_bits.cpu().tolist() == [blk.bits for _, _, blk, _ in chunks]
    for k, (_, _, blk, _) in enumerate(chunks):
        assert np.array_equal(_u32(codes[k]), blk.code_table()), (name, k)
        assert np.array_equal(_u32(header[k]), blk.header_words()), (name, k)
    slots = ops.png_emit(tokens, ntok, codes, header, header_bits).cpu().numpy()
    for k, (_, _, blk, bits) in enumerate(chunks):
        raw = bits.tobytes()
        assert slots[k, :len(raw)].tobytes() == raw and not slots[k, len(raw):].any(), (name, k)
    chunk_off, frame_bytes = ops.png_pack_scan(chunk_bits, 1)
    assert chunk_off.cpu().tolist() == np.concatenate([[0], np.cumsum([blk.bits for _, _, blk, _ in chunks])[:-1]]).tolist()
    assert frame_bytes.cpu().tolist() == [len(stream) - 6]
    packed = ops.png_pack(_dev(slots), chunk_bits, chunk_off, 1, len(stream) - 6)
    assert packed.cpu().numpy().tobytes() == stream[2:-4]
    assert ops.png_adler(filtered).cpu().tolist() == [zlib.adler32(data)]
    assert P.encode_filtered(filtered) == [stream]


@pytest.mark.parametrize("name", ["fibonacci", "codelengths"])
def test_codes_and_emit_on_crafted_tokens(name):
    """Tokens and histograms the token stage would never produce, fed to the codes and emit stages directly: the length limits 15 and 7
    are reached (tests/test_png.py asserts that the unlimited trees are deeper) and the bits are the restatement's."""
    _need_gpu()
    from ccedit_amd import ops
    tok, hist = K.token_cases()[name]
    blk = M.Block(hist, True)
    assert (blk.lit_unlimited > P.MAX_BITS) if name == "fibonacci" else (blk.cl_unlimited > P.CL_MAX_BITS)
    codes, header, header_bits, chunk_bits = ops.png_codes(_words(hist[None]), 1)
    assert np.array_equal(_u32(codes[0]), blk.code_table()) and np.array_equal(_u32(header[0]), blk.header_words())
    assert header_bits.cpu().tolist() == [blk.header.n] and chunk_bits.cpu().tolist() == [blk.bits]
    padded = np.zeros((1, P.CHUNK), dtype=np.uint32)
    padded[0, :len(tok)] = tok
    ntok = torch.tensor([len(tok)], dtype=torch.int32, device="cuda")
    slots = ops.png_emit(_words(padded), ntok, codes, header, header_bits).cpu().numpy()
    raw = blk.emit(tok).tobytes()
    assert slots[0, :len(raw)].tobytes() == raw and not slots[0, len(raw):].any()


def test_first_and_last_chunk_flags_of_several_streams():
    """N = 3 streams of 2 CHUNK + 1 bytes in one launch: BFINAL on each stream's last chunk only, offsets continue over the streams."""
    _need_gpu()
    data = K.streams()["noise"]
    rolled = [data, data[1:] + data[:1], data[::-1]]
    got = P.encode_filtered(_dev(np.stack([np.frombuffer(d, dtype=np.uint8) for d in rolled])))
    assert got == [M.zlib_stream(d) for d in rolled]


# ---- 2. frames to files ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", K.CONTENTS)
def test_files_equal_the_restatement(tmp_path, kind):
    _need_gpu()
    frames = np.stack([K.frame(kind, 64, 96, s) for s in range(3)])
    got = _device_file(tmp_path, frames, 333)
    assert got == _mirror_file(tmp_path, frames, 333)
    im, decoded = pillow_frames(str(tmp_path / "got.png"))
    assert im.n_frames == 3 and im.info["duration"] == 333.0 and (decoded == frames).all()


@pytest.mark.parametrize("h,w", K.SMALL_SHAPES[:-1] + list(K.BORDER_SHAPES.values()))
def test_files_equal_the_restatement_over_the_shapes(tmp_path, h, w):
    _need_gpu()
    frames = K.clip(h, w, 2)
    assert _device_file(tmp_path, frames, 50) == _mirror_file(tmp_path, frames, 50)


def test_one_frame_and_full_size(tmp_path):
    """A single frame is a plain PNG; two frames of 512 x 768 (73 chunks each): a photo-like frame and a ramp."""
    _need_gpu()
    one = K.clip(33, 50, 1)
    assert _device_file(tmp_path, one, 50) == _mirror_file(tmp_path, one, 50)
    frames = np.stack([K.frame("photo", 512, 768, 1), K.frame("ramp", 512, 768, 2)])
    assert _device_file(tmp_path, frames, 50) == _mirror_file(tmp_path, frames, 50)
    assert (pillow_frames(str(tmp_path / "got.png"))[1] == frames).all()


def test_more_frames_than_one_launch(tmp_path, monkeypatch):
    """N = 65 at 17 x 19: two launch groups (64 + 1); and the scratch bound does not change a byte."""
    _need_gpu()
    assert P.frames_per_launch(17, 19) == 64
    frames = K.clip(17, 19, 65)
    want = _mirror_file(tmp_path, frames, 50)
    assert _device_file(tmp_path, frames, 50) == want
    monkeypatch.setattr(P, "MAX_FRAMES_PER_LAUNCH", 7)
    assert _device_file(tmp_path, frames, 50) == want


def test_ops_refuse_bad_arguments():
    _need_gpu()
    from ccedit_amd import ops
    ok = _dev(np.zeros((1, 8, 8, 3), np.uint8))
    for bad in (ok.cpu(), ok.float(), ok[0], ok[..., :2], ok.permute(0, 2, 1, 3)):
        with pytest.raises(ValueError):
            ops.png_filter(bad)
    with pytest.raises(ValueError):
        ops.png_tokens(ops.png_filter(ok))                                  # (N, H, 1 + 3 W): the stages take (N, L)
    hist = ops.png_tokens(ops.png_filter(ok).reshape(1, -1))[2]
    with pytest.raises(ValueError):
        ops.png_codes(hist, 2)
    with pytest.raises(ValueError):
        ops.png_codes(hist[:, :100].contiguous(), 1)
    with pytest.raises(ValueError):
        ops.png_pack_scan(torch.zeros(3, dtype=torch.int32, device="cuda"), 2)


# ---- 3. the entry level --------------------------------------------------------------------------------
def test_save_numbers_files_and_both_routes_write_the_same_bytes(tmp_path):
    _need_gpu()
    from scripts.sampling.util import perform_save_locally_video
    g = torch.Generator().manual_seed(2)
    x = torch.rand(2, 3, 4, 33, 50, generator=g)
    host, dev = str(tmp_path / "host"), str(tmp_path / "dev")
    p0 = perform_save_locally_video(host, x, 5, "png", return_savepaths=True)
    p1 = perform_save_locally_video(host, x[:1, :, :1], 5, "png", return_savepaths=True, save_grid=False, video_quality=40)
    assert p0 == [os.path.join(host, "png", f"animation-{i:04}.png") for i in range(2)]
    assert p1 == [os.path.join(host, "png", "animation-0002.png")]
    assert sorted(os.listdir(os.path.join(host, "grid"))) == ["grid-0000.png", "grid-0001.png"]
    p2 = perform_save_locally_video(dev, x.cuda(), 5, "png", return_savepaths=True, gpu_io=True)
    assert [open(p, "rb").read() for p in p2] == [open(p, "rb").read() for p in p0]
    p3 = perform_save_locally_video(dev, (x * 2 - 1).cuda(), 5, "png", return_savepaths=True, gpu_io=True, signed=True, save_grid=False)
    assert len(p3) == 2
    for b in range(2):                                                      # the gif branch's uint8 frames, exactly
        u8 = (255.0 * x[b].permute(1, 2, 3, 0).numpy()).astype(np.uint8)
        im, got = pillow_frames(p0[b])
        assert im.n_frames == 4 and im.info["duration"] == 200.0 and (got == u8).all()
        assert open(p0[b], "rb").read() == open(M.write_apng(str(tmp_path / "m.png"), u8, 200), "rb").read()
    assert getattr(Image.open(p1[0]), "n_frames", 1) == 1                   # one frame: a plain PNG


def _write_config(tmp_path):
    import yaml
    from ccedit_amd.sgm_compat import engine_config
    cfg = os.path.join(str(tmp_path), "tv2v.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump(dict(model=engine_config(crossframe=False, vae_ch=32, model_channels=64, num_heads=2, context_dim=64)), f)
    return cfg


@pytest.mark.timeout(900)
def test_entry_point_writes_animated_png(tmp_path, monkeypatch):
    """sampling_tv2v.py --synthetic --save_type png --propagate on a frame directory of 7 frames, 3 keyframes at gap 3, at the smallest
    shape of the entry-point tests (64 x 128), with and without --gpu_io: the files of the two routes are byte-identical, the paths of
    log_info.json exist, and every frame of result/ decodes to (255 * x).astype(uint8) of what --save_type npy writes for the same job."""
    _need_gpu()
    from _gif_cases import smoothed
    from scripts.sampling import sampling_tv2v as S
    from scripts.sampling import util as U
    cfg = _write_config(tmp_path)
    vdir = tmp_path / "clips" / "fox"
    vdir.mkdir(parents=True)
    big = smoothed(90 + 20, 150 + 20, 30)
    for i in range(7):
        Image.fromarray(big[i:i + 90, 2 * i:2 * i + 150]).save(str(vdir / f"{i:03d}.png"))
    base = ["sampling_tv2v.py", "--config_path", cfg, "--synthetic", "--H", "64", "--W", "128", "--num_keyframes", "3", "--sample_steps", "2",
            "--sampler_name", "DPMPP2SAncestralSampler", "--original_fps", "9", "--target_fps", "3", "--noise_seed", "1", "--prompt", "a red fox",
            "--video_path", str(vdir), "--batch_size", "1"]
    logs = {}
    try:
        for tag, extra in (("host", ["--save_type", "png", "--propagate"]), ("device", ["--save_type", "png", "--propagate", "--gpu_io"]),
                           ("npy", ["--save_type", "npy"])):
            out = str(tmp_path / tag)
            monkeypatch.setattr(sys, "argv", base + ["--save_path", out] + extra)
            S.main()
            logs[tag] = json.load(open(os.path.join(out, "default", "log_info.json")))
    finally:
        torch.set_grad_enabled(True)
    for tag in ("host", "device"):
        out = str(tmp_path / tag)
        assert logs[tag]["keyframes_paths"] == [os.path.join(out, "default", "result", "png", "animation-0000.png")]
        assert logs[tag]["fullrate_paths"] == [os.path.join(out, "default", "result_full", "png", "animation-0000.png")]
        for kind in ("original", "result", "control_hint"):
            assert os.listdir(os.path.join(out, "default", kind)) == ["png"]
    for kind in ("keyframes_paths", "fullrate_paths"):
        assert os.path.exists(logs["host"][kind][0])
        assert open(logs["host"][kind][0], "rb").read() == open(logs["device"][kind][0], "rb").read(), f"{kind}: the two I/O routes differ"
    for kind in ("original", "control_hint"):
        a, b = (open(os.path.join(str(tmp_path / t), "default", kind, "png", "animation-0000.png"), "rb").read() for t in ("host", "device"))
        assert a == b, kind
    im, keys = pillow_frames(logs["host"]["keyframes_paths"][0])
    assert im.n_frames == 3 and im.info["duration"] == 333.0 and keys.shape == (3, 64, 128, 3)
    x = np.load(logs["npy"]["keyframes_paths"][0])
    assert x.shape == (3, 64, 128, 3) and (keys == (255.0 * x).astype(np.uint8)).all()
    im, full = pillow_frames(logs["host"]["fullrate_paths"][0])
    assert im.n_frames == 7 and im.info["duration"] == 111.0 and (full[0::3] == keys).all()
    # the written file is a source of the next run
    assert U.count_video_frames(logs["host"]["fullrate_paths"][0]) == 7
    kf = U.load_video_keyframes(logs["host"]["fullrate_paths"][0], 9, 3, 3, (64, 128), device=torch.device("cuda"))
    assert tuple(kf.shape) == (3, 3, 64, 128)
