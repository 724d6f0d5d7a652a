"""The routing of the frame / video I/O (scripts/sampling/util.py and its callers in sampling_tv2v.py), pinned through the public
functions alone and without a device: every source kind goes to the decoder, the resize and the stderr line it always went to, every
writer puts its file where it always did.  The device decoders and encoders and the `ops` functions are stood in for by recorders that
return CPU tensors of the right shape; a "device" is torch.device("cpu"), and where a writer uploads a host array the upload is stood in
for by a tensor that calls itself a device tensor.  Frames are 16 x 24; the Motion-JPEG clips are 16 x 32 (write_avi takes whole 16 x 16
MCUs only)."""
import io
import os
import types

import numpy as np
import pytest
import torch
from PIL import Image

import _mjpeg_numpy as RJ
import _png_numpy as RP
from ccedit_amd import gif, jpegdec, mjpeg, ops, png, pngdec
from scripts.sampling import sampling_tv2v as S
from scripts.sampling import util as U

H, W, WA = 16, 24, 32
CPU = torch.device("cpu")
TAIL = "; this clip is decoded by Pillow on the host\n"
UNSUPPORTED = "Unsupported video format. Only support dirctory, .mp4, .gif and .avi (Motion-JPEG)."
MP4 = ("mp4 decoding needs decord / cv2 / imageio-ffmpeg, none of which is installed; "
       "extract the frames to a directory of images (or a .gif) instead")


def _frame(i, h=H, w=W):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(xx * 9 + 40 * i) % 256, (yy * 13 + 25 * i) % 256, (xx * yy + 60 * i) % 256], -1).astype(np.uint8)


class _Sources:
    def __init__(self, root):
        self.root = str(root)
        self.frames = [_frame(i) for i in range(6)]

    def path(self, *parts):
        return os.path.join(self.root, *parts)

    def folder(self, name, files):
        """files: (file name, PIL image, save options) in order"""
        os.makedirs(self.path(name))
        for fname, img, opts in files:
            img.save(self.path(name, fname), **opts)
        return self.path(name)

    def data(self, name, picks=None):
        files = sorted(os.listdir(self.path(name)))
        return tuple(open(self.path(name, files[i]), "rb").read() for i in (range(len(files)) if picks is None else picks))


@pytest.fixture(scope="module")
def src(tmp_path_factory):
    s = _Sources(tmp_path_factory.mktemp("routes"))
    img = [Image.fromarray(f) for f in s.frames]
    small = Image.fromarray(_frame(2, 8, W))
    s.folder("jpg", [(f"{i:03d}.{'JPEG' if i == 3 else 'jpg'}", img[i], {}) for i in range(6)])
    s.folder("png", [(f"{i:03d}.{'PNG' if i == 2 else 'png'}", img[i], {}) for i in range(6)])
    s.folder("mixed", [(f"{i:03d}.{'jpg' if i % 2 else 'png'}", img[i], {}) for i in range(4)])
    s.folder("sizes_png", [(f"{i:03d}.png", small if i == 2 else img[i], {}) for i in range(4)])
    s.folder("sizes_jpg", [(f"{i:03d}.jpg", small if i == 2 else img[i], {}) for i in range(4)])
    s.folder("progressive", [(f"{i:03d}.jpg", img[i], dict(progressive=True) if i == 1 else {}) for i in range(4)])
    s.folder("rgba", [(f"{i:03d}.png", img[i].convert("RGBA") if i == 1 else img[i], {}) for i in range(4)])
    s.folder("grey", [(f"{i:03d}.jpg", img[i].convert("L") if i == 2 else img[i], {}) for i in range(4)])
    flat = [Image.fromarray((f // 64 * 64).astype(np.uint8)) for f in s.frames]
    flat[0].save(s.path("clip.gif"), save_all=True, append_images=flat[1:], duration=100, loop=0)
    wide = np.stack([_frame(i, H, WA) for i in range(6)])
    s.avi_jpegs = RJ.encode_frames(wide, 90)
    mjpeg.write_avi(s.path("clip.avi"), s.avi_jpegs, 6, H, WA)
    progressive = []
    for i in range(4):
        b = io.BytesIO()
        Image.fromarray(wide[i]).save(b, "JPEG", progressive=(i == 1))
        progressive.append(b.getvalue())
    mjpeg.write_avi(s.path("progressive.avi"), progressive, 6, H, WA)
    s.avi_progressive = progressive
    png.write_apng(s.path("clip.png"), RP.encode_frames(np.stack(s.frames)), 100, W, H)
    s.apng_streams = pngdec.parse(open(s.path("clip.png"), "rb").read()).frames
    rgba = [i.convert("RGBA") for i in img[:4]]
    rgba[0].save(s.path("rgba_clip.png"), save_all=True, append_images=rgba[1:], duration=100, loop=0)
    img[0].save(s.path("still.png"))
    return s


class _Recorder:
    """Stands in for the device decoders and the ops functions of the loaders; `calls` is what ran, in order."""

    def __init__(self, monkeypatch):
        self.calls = []
        self.fail = {}                      # name of a decoder -> f(the byte strings of the call) -> an exception to raise, or None
        monkeypatch.setattr(jpegdec, "decode", lambda jpegs, device, infos=None: self._files("jpegdec.decode", jpegs, device, infos))
        monkeypatch.setattr(pngdec, "decode", lambda datas, device, infos=None: self._files("pngdec.decode", datas, device, infos))
        monkeypatch.setattr(pngdec, "decode_streams", self._streams)
        monkeypatch.setattr(ops, "resize_u8_pil", self._resize_u8_pil)
        monkeypatch.setattr(ops, "resize_bicubic", self._resize_bicubic)
        monkeypatch.setattr(ops, "frames_to_u8", self._frames_to_u8)
        monkeypatch.setattr(ops, "mask_resize_nearest", self._mask_resize_nearest)

    def take(self):
        out, self.calls = self.calls, []
        return out

    def _raise(self, name, datas):
        e = self.fail.get(name, lambda d: None)(datas)
        if e is not None:
            raise e

    def _files(self, name, datas, device, infos):
        assert device == CPU and infos is not None and len(infos) == len(datas)          # (each file was parsed once, by the router)
        self.calls.append((name, tuple(datas)))
        self._raise(name, tuple(datas))
        return torch.zeros((len(datas), infos[0].height, infos[0].width, 3), dtype=torch.uint8)

    def _streams(self, streams, h, w, device, check=True):
        assert device == CPU and check
        self.calls.append(("pngdec.decode_streams", tuple(streams)))
        self._raise("pngdec.decode_streams", tuple(streams))
        return torch.zeros((len(streams), h, w, 3), dtype=torch.uint8), np.zeros((len(streams), 2), np.int32)

    def _resize_u8_pil(self, x, size, to_float=False):
        assert x.dtype == torch.uint8 and x.is_contiguous()
        n, (h, w) = x.shape[0], size
        self.calls.append(("resize_u8_pil", tuple(x.shape), (int(h), int(w)), bool(to_float)))
        return torch.zeros((3, n, h, w)) if to_float else torch.zeros((n, h, w, 3), dtype=torch.uint8)

    def _resize_bicubic(self, x, size):
        assert x.dtype == torch.float32 and x.is_contiguous()
        self.calls.append(("resize_bicubic", tuple(x.shape), tuple(size)))
        return torch.zeros((x.shape[0], x.shape[1], size[0], size[1]))

    def _frames_to_u8(self, x, rounding=False, unit_range=False):
        assert x.dtype == torch.float32 and x.is_contiguous()
        self.calls.append(("frames_to_u8", tuple(x.shape), bool(rounding), bool(unit_range)))
        b, _, t, h, w = x.shape
        return torch.zeros((b, t, h, w, 3), dtype=torch.uint8).as_subclass(type(x))

    def _mask_resize_nearest(self, m, size):
        assert m.dtype == torch.uint8 and m.is_contiguous()
        self.calls.append(("mask_resize_nearest", tuple(m.shape), tuple(size)))
        return torch.zeros((m.shape[0], size[0], size[1]), dtype=torch.uint8)


@pytest.fixture
def rec(monkeypatch):
    return _Recorder(monkeypatch)


def _every(n):
    """original_fps, target_fps, num_keyframes that select every one of n frames"""
    return 4, 4, n


# ---- frame directories and single image files
@pytest.mark.parametrize("name,decoder", [("jpg", "jpegdec.decode"), ("png", "pngdec.decode")])
def test_a_directory_of_one_codec_is_decoded_in_one_batch(src, rec, capsys, name, decoder):
    d = src.path(name)
    x = U.load_video_keyframes(d, 6, 3, 3, size=(8, 12), device=CPU)                       # every second file: 0, 2, 4
    assert rec.take() == [(decoder, src.data(name, (0, 2, 4))), ("resize_u8_pil", (3, H, W, 3), (8, 12), True)]
    assert x.shape == (3, 3, 8, 12) and x.dtype == torch.float32
    x = U.load_video_keyframes(d, 6, 3, 3, device=CPU)                                     # no size: the "resize" is the float conversion
    assert rec.take() == [(decoder, src.data(name, (0, 2, 4))), ("resize_u8_pil", (3, H, W, 3), (H, W), True)] and x.shape == (3, 3, H, W)
    x = U.load_video_frames_u8(d, (8, 12), CPU)
    assert rec.take() == [(decoder, src.data(name)), ("resize_u8_pil", (6, H, W, 3), (8, 12), False)]
    assert x.shape == (6, 8, 12, 3) and x.dtype == torch.uint8
    one = os.path.join(d, sorted(os.listdir(d))[3])
    x = U.load_img(one, (8, 12), device=CPU)
    assert rec.take() == [(decoder, src.data(name, (3,))), ("resize_u8_pil", (1, H, W, 3), (8, 12), True)] and x.shape == (1, 3, 8, 12)
    assert U.count_video_frames(d) == 6
    assert capsys.readouterr().err == ""


def test_the_host_route_calls_nothing_of_the_device(src, rec, capsys):
    for name in ("jpg", "png", "mixed", "progressive"):
        n = len(os.listdir(src.path(name)))
        x = U.load_video_keyframes(src.path(name), *_every(n), size=(8, 12))
        assert x.shape == (n, 3, 8, 12) and float(x.min()) >= -1.0 and float(x.max()) <= 1.0
    assert U.load_img(src.path("still.png"), (8, 12)).shape == (1, 3, 8, 12)
    want = torch.from_numpy(np.stack(src.frames)[[0, 2, 4]]).permute(0, 3, 1, 2).float() / 255.0 * 2.0 - 1.0
    assert torch.equal(U.load_video_keyframes(src.path("png"), 6, 3, 3), want)
    assert torch.equal(U.load_video_keyframes(src.path("clip.png"), 6, 3, 3), want)       # (lossless: the animated PNG holds the same bytes)
    assert U.load_video_keyframes(src.path("clip.gif"), 6, 3, 3, size=(8, 12)).shape == (3, 3, 8, 12)
    assert U.load_video_keyframes(src.path("clip.avi"), 6, 3, 3, size=(8, 12)).shape == (3, 3, 8, 12)
    assert rec.take() == [] and capsys.readouterr().err == ""


def test_mixed_extensions_go_through_pillow_without_a_word(src, rec, capsys):
    d = src.path("mixed")
    assert U.load_video_keyframes(d, *_every(4), size=(8, 12), device=CPU).shape == (4, 3, 8, 12)
    assert rec.take() == [("resize_u8_pil", (4, H, W, 3), (8, 12), True)]                 # Pillow's frames, uploaded as one stack
    assert U.load_video_frames_u8(d, (8, 12), CPU).shape == (4, 8, 12, 3)
    assert rec.take() == [("resize_u8_pil", (4, H, W, 3), (8, 12), False)]
    assert capsys.readouterr().err == "" and U.count_video_frames(d) == 4


@pytest.mark.parametrize("name,decoder", [("sizes_jpg", "jpegdec.decode"), ("sizes_png", "pngdec.decode")])
def test_two_sizes_make_one_call_per_file_and_need_a_size(src, rec, capsys, name, decoder):
    d, data = src.path(name), src.data(name)
    shapes = [(1, 8 if i == 2 else H, W, 3) for i in range(4)]
    x = U.load_video_keyframes(d, *_every(4), size=(8, 12), device=CPU)
    assert rec.take() == [(decoder, (data[i],)) for i in range(4)] + [("resize_u8_pil", s, (8, 12), True) for s in shapes]
    assert x.shape == (4, 3, 8, 12)
    x = U.load_video_frames_u8(d, (8, 12), CPU)
    assert rec.take() == [(decoder, (data[i],)) for i in range(4)] + [("resize_u8_pil", s, (8, 12), False) for s in shapes]
    assert x.shape == (4, 8, 12, 3)
    with pytest.raises(AssertionError, match="frames of different sizes need a target size"):
        U.load_video_keyframes(d, *_every(4), device=CPU)
    assert capsys.readouterr().err == ""


def test_a_file_the_parser_refuses_sends_the_whole_clip_to_pillow_with_one_line(src, rec, capsys):
    d = src.path("progressive")
    with pytest.raises(jpegdec.JpegUnsupported) as why:
        jpegdec.parse(src.data("progressive", (1,))[0])
    line = f"[jpegdec] {d}: 001.jpg: {why.value}{TAIL}"
    assert U.load_video_keyframes(d, *_every(4), size=(8, 12), device=CPU).shape == (4, 3, 8, 12)
    assert rec.take() == [("resize_u8_pil", (4, H, W, 3), (8, 12), True)] and capsys.readouterr().err == line
    assert U.load_video_frames_u8(d, (8, 12), CPU).shape == (4, 8, 12, 3)
    assert rec.take() == [("resize_u8_pil", (4, H, W, 3), (8, 12), False)] and capsys.readouterr().err == line
    one = os.path.join(d, "001.jpg")
    assert U.load_img(one, (8, 12), device=CPU).shape == (1, 3, 8, 12)
    assert rec.take() == [("resize_u8_pil", (1, H, W, 3), (8, 12), True)]
    assert capsys.readouterr().err == f"[jpegdec] {one}: 001.jpg: {why.value}{TAIL}"
    assert U.load_video_keyframes(d, 4, 2, 2, size=(8, 12), device=CPU).shape == (2, 3, 8, 12)       # files 0 and 2: the refused one is not read
    assert rec.take() == [("jpegdec.decode", src.data("progressive", (0, 2))), ("resize_u8_pil", (2, H, W, 3), (8, 12), True)]
    assert capsys.readouterr().err == ""
    # PNG: RGBA is outside the subset; Pillow's route then refuses it too, as it always did on the device route
    d = src.path("rgba")
    with pytest.raises(pngdec.PngUnsupported) as why:
        pngdec.parse(src.data("rgba", (1,))[0])
    with pytest.raises(ValueError, match="the device route takes 8-bit RGB images"):
        U.load_video_frames_u8(d, (8, 12), CPU)
    assert rec.take() == [] and capsys.readouterr().err == f"[pngdec] {d}: 001.png: {why.value}{TAIL}"
    # a greyscale JPEG parses, but is no three-component image: declined silently
    with pytest.raises(ValueError, match="the device route takes 8-bit RGB images"):
        U.load_video_frames_u8(src.path("grey"), (8, 12), CPU)
    assert rec.take() == [] and capsys.readouterr().err == ""


def test_a_png_any_value_error_of_the_parser_declines_a_jpeg_only_its_own(src, rec, capsys, tmp_path, monkeypatch):
    data = src.data("png", (0,))[0]
    (tmp_path / "000.png").write_bytes(data[:50] + bytes([data[50] ^ 4]) + data[51:])           # a bad CRC: a plain ValueError
    with pytest.raises(Exception):                                                               # (Pillow does not take the file either)
        U.load_video_frames_u8(str(tmp_path), (8, 12), CPU)
    err = capsys.readouterr().err
    assert err.startswith(f"[pngdec] {tmp_path}: 000.png: bad CRC") and err.endswith(TAIL) and err.count("\n") == 1 and rec.take() == []

    def broken(data):
        raise ValueError("not the parser's own refusal")
    monkeypatch.setattr(jpegdec, "parse", broken)
    with pytest.raises(ValueError, match="^not the parser's own refusal$"):
        U.load_video_frames_u8(src.path("jpg"), (8, 12), CPU)
    assert rec.take() == [] and capsys.readouterr().err == ""


def test_a_device_status_is_reworded_per_route(src, rec):
    boom = "frame 1, restart interval 0: boom"
    rec.fail["jpegdec.decode"] = lambda datas: ValueError(boom)
    d = src.path("jpg")
    with pytest.raises(ValueError) as e:
        U.load_video_frames_u8(d, (8, 12), CPU)
    assert str(e.value) == f"{d}: {boom}" and type(e.value) is ValueError
    avi = src.path("clip.avi")
    with pytest.raises(ValueError) as e:
        U.load_video_frames_u8(avi, (8, 12), CPU)
    assert str(e.value) == f"{avi}: {boom}"
    with pytest.raises(ValueError) as e:
        U.load_video_keyframes(avi, 6, 3, 3, size=(8, 12), device=CPU)
    assert str(e.value) == f"{avi}: selected {boom}"
    rec.fail["jpegdec.decode"] = lambda datas: jpegdec.JpegUnsupported("late refusal")
    with pytest.raises(jpegdec.JpegUnsupported, match="^late refusal$"):
        U.load_video_frames_u8(d, (8, 12), CPU)
    # PNG files: the frame is counted in the clip, in the one-batch call and in the call-per-file case
    stopped = "Adler-32 mismatch (code 11 at byte 77)"
    d, data = src.path("png"), src.data("png")
    rec.fail["pngdec.decode"] = lambda datas: ValueError(f"frame {datas.index(data[2])}: {stopped}") if data[2] in datas else None
    with pytest.raises(ValueError) as e:
        U.load_video_frames_u8(d, (8, 12), CPU)
    assert str(e.value) == f"{d}: 002.PNG: frame 2: {stopped}"
    with pytest.raises(ValueError) as e:
        U.load_video_keyframes(d, 6, 3, 3, device=CPU)                                          # files 0, 2, 4: the clip's frame 1
    assert str(e.value) == f"{d}: 002.PNG: frame 1: {stopped}"
    d, data = src.path("sizes_png"), src.data("sizes_png")
    with pytest.raises(ValueError) as e:
        U.load_video_frames_u8(d, (8, 12), CPU)
    assert str(e.value) == f"{d}: 002.png: frame 2: {stopped}"
    rec.fail["pngdec.decode"] = lambda datas: ValueError("decode: something else")
    with pytest.raises(ValueError) as e:
        U.load_video_frames_u8(d, (8, 12), CPU)
    assert str(e.value) == f"{d}: decode: something else"
    # animated PNG: the path in front, the frame mapped back through the selection
    anim = src.path("clip.png")
    rec.fail["pngdec.decode_streams"] = lambda streams: pngdec.status_error(11, 77, 1)
    with pytest.raises(ValueError) as e:
        U.load_video_keyframes(anim, 6, 3, 3, device=CPU)
    assert str(e.value) == f"{anim}: frame 2: {stopped}"
    with pytest.raises(ValueError) as e:
        U.load_video_frames_u8(anim, (8, 12), CPU)
    assert str(e.value) == f"{anim}: frame 1: {stopped}"


# ---- videos held in one file
def test_single_file_videos_decode_the_selected_frames_and_resize_in_float(src, rec, capsys):
    cases = [("clip.avi", "jpegdec.decode", src.avi_jpegs, WA), ("clip.png", "pngdec.decode_streams", src.apng_streams, W)]
    for name, decoder, frames, w in cases:
        path = src.path(name)
        x = U.load_video_keyframes(path, 6, 3, 3, size=(8, 12), device=CPU)
        assert rec.take() == [(decoder, tuple(frames[i] for i in (0, 2, 4))), ("resize_u8_pil", (3, H, w, 3), (H, w), True),
                              ("resize_bicubic", (3, 3, H, w), (8, 12))]
        assert x.shape == (3, 3, 8, 12)
        x = U.load_video_keyframes(path, 6, 3, 3, device=CPU)
        assert rec.take() == [(decoder, tuple(frames[i] for i in (0, 2, 4))), ("resize_u8_pil", (3, H, w, 3), (H, w), True)]
        assert x.shape == (3, 3, H, w)
        x = U.load_video_frames_u8(path, (8, 12), CPU)
        assert rec.take() == [(decoder, tuple(frames)), ("resize_u8_pil", (6, H, w, 3), (H, w), True), ("resize_bicubic", (6, 3, H, w), (8, 12)),
                              ("frames_to_u8", (1, 3, 6, 8, 12), True, False)]
        assert x.shape == (6, 8, 12, 3) and U.count_video_frames(path) == 6
    # a .gif has no device decoder: Pillow's frames, the keyframes selected before the upload
    path = src.path("clip.gif")
    assert U.load_video_keyframes(path, 6, 3, 3, size=(8, 12), device=CPU).shape == (3, 3, 8, 12)
    assert rec.take() == [("resize_u8_pil", (3, H, W, 3), (H, W), True), ("resize_bicubic", (3, 3, H, W), (8, 12))]
    assert U.load_video_frames_u8(path, (8, 12), CPU).shape == (6, 8, 12, 3)
    assert rec.take() == [("resize_u8_pil", (6, H, W, 3), (H, W), True), ("resize_bicubic", (6, 3, H, W), (8, 12)),
                          ("frames_to_u8", (1, 3, 6, 8, 12), True, False)]
    assert U.count_video_frames(path) == 6 and capsys.readouterr().err == ""


def test_single_file_videos_the_parser_refuses_go_through_pillow_with_one_line(src, rec, capsys):
    path = src.path("progressive.avi")
    with pytest.raises(jpegdec.JpegUnsupported) as why:
        jpegdec.parse(src.avi_progressive[1])
    for select in (True, False):                    # frame 1 is not among the keyframes 0 and 2: the clip goes one way as a whole all the same
        if select:
            assert U.load_video_keyframes(path, 4, 2, 2, size=(8, 12), device=CPU).shape == (2, 3, 8, 12)
            assert rec.take() == [("resize_u8_pil", (2, H, WA, 3), (H, WA), True), ("resize_bicubic", (2, 3, H, WA), (8, 12))]
        else:
            assert U.load_video_frames_u8(path, (8, 12), CPU).shape == (4, 8, 12, 3)
            assert [c[0] for c in rec.take()] == ["resize_u8_pil", "resize_bicubic", "frames_to_u8"]
        assert capsys.readouterr().err == f"[jpegdec] {path}: frame 1: {why.value}{TAIL}"
    path = src.path("rgba_clip.png")
    with pytest.raises(pngdec.PngUnsupported) as why:
        pngdec.parse(open(path, "rb").read())
    assert U.load_video_keyframes(path, 4, 2, 2, size=(8, 12), device=CPU).shape == (2, 3, 8, 12)
    assert rec.take() == [("resize_u8_pil", (2, H, W, 3), (H, W), True), ("resize_bicubic", (2, 3, H, W), (8, 12))]
    assert capsys.readouterr().err == f"[pngdec] {path}: {why.value}{TAIL}"
    assert U.count_video_frames(path) == 4


def test_what_is_no_video_says_so_in_one_of_two_ways(src, rec):
    for path in (src.path("still.png"), src.path("absent.png"), "clip.xyz", "clip.GIF", "clip.AVI"):
        for call in (lambda: U.load_video_keyframes(path, 6, 3, 3), lambda: U.load_video_keyframes(path, 6, 3, 3, device=CPU),
                     lambda: U.load_video_frames_u8(path, (8, 12), CPU), lambda: U.count_video_frames(path)):
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == UNSUPPORTED
    for call in (lambda: U.load_video_keyframes("clip.mp4", 6, 3, 3), lambda: U.load_video_frames_u8("clip.mp4", (8, 12), CPU)):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == MP4
    with pytest.raises(ValueError) as e:
        U.count_video_frames("clip.mp4")
    assert str(e.value) == UNSUPPORTED and rec.take() == []


def test_masks_stay_on_pillow_for_every_kind(src, rec, capsys):
    for name, n, w in (("jpg", 6, W), ("png", 6, W), ("mixed", 4, W), ("clip.gif", 6, W), ("clip.avi", 6, WA), ("clip.png", 6, W)):
        path = src.path(name)
        m = U.load_video_mask(path, *_every(n), size=(8, 12), num_allframes=n)
        assert m.shape == (n, 8, 12) and m.dtype == torch.uint8 and set(np.unique(m.numpy())) <= {0, 255} and rec.take() == []
        assert U.load_video_mask(path, n, n // 2, 2, num_allframes=n).shape == (2, H, w)
        m = U.load_video_mask(path, n, n // 2, 2, size=(8, 12), num_allframes=n, device=CPU)
        assert rec.take() == [("mask_resize_nearest", (2, H, w), (8, 12))] and m.shape == (2, 8, 12)
        m = U.load_video_mask(path, n, n // 2, 2, size=(8, 12), num_allframes=n, device=CPU, all_frames=True)
        assert rec.take() == [("mask_resize_nearest", (n, H, w), (8, 12))] and m.shape == (n, 8, 12)
        with pytest.raises(ValueError, match=f"has {n} frames, the video has {n + 1}"):
            U.load_video_mask(path, *_every(n), num_allframes=n + 1)
    one = U.load_video_mask(src.path("still.png"), 6, 3, 3, num_allframes=17)                 # ONE image: used for every keyframe
    assert one.shape == (3, H, W) and torch.equal(one[0], one[2]) and rec.take() == []
    assert U.load_video_mask(src.path("still.png"), 6, 3, 3, num_allframes=5, all_frames=True).shape == (5, H, W)
    with pytest.raises(ValueError, match="needs num_allframes"):
        U.load_video_mask(src.path("still.png"), 6, 3, 3, all_frames=True)
    with pytest.raises(ValueError) as e:
        U.load_video_mask("mask.mp4", 6, 3, 3)
    assert str(e.value) == ("Unsupported mask format: mask.mp4. Only support directory, .gif, .avi (Motion-JPEG) and one image file "
                            "('.png', '.jpg', '.jpeg', '.bmp', '.webp', '.tif', '.tiff').")
    assert capsys.readouterr().err == ""


# ---- writers
class _OnDevice(torch.Tensor):
    """A CPU tensor that calls itself a device tensor: what an upload gives, where there is no device."""
    is_cuda = property(lambda self: True)


class _Encoders:
    """Stands in for the three device encoders; each returns fixed byte strings, the containers around them are the real ones."""
    PALETTE, LZW, ZLIB, JPEG = bytes(range(256)) * 3, b"\x00\x01\x02", b"\x78\x01" + bytes(10), b"\xff\xd8fixed\xff\xd9"

    def __init__(self, monkeypatch):
        self.calls = []
        real = torch.from_numpy
        monkeypatch.setattr(torch, "from_numpy", lambda a: real(a).as_subclass(_OnDevice))      # (a host array is "uploaded": see above)
        monkeypatch.setattr(gif, "encode_frames", lambda frames: self._take("gif", frames, [(self.PALETTE, self.LZW)]))
        monkeypatch.setattr(png, "encode_frames", lambda frames: self._take("png", frames, [self.ZLIB]))
        monkeypatch.setattr(mjpeg, "encode_frames", lambda frames, quality=90: self._take("mjpeg", frames, [self.JPEG], quality))
        monkeypatch.setattr(ops, "frames_to_u8", self._frames_to_u8)

    def take(self):
        out, self.calls = self.calls, []
        return out

    def _take(self, name, frames, per_frame, *options):
        assert torch.is_tensor(frames) and frames.is_cuda and frames.dtype == torch.uint8 and frames.is_contiguous()
        self.calls.append((name, tuple(frames.shape)) + options)
        return per_frame * frames.shape[0]

    def _frames_to_u8(self, x, rounding=False, unit_range=False):
        self.calls.append(("frames_to_u8", bool(rounding), bool(unit_range)))
        b, _, t, h, w = x.shape                                                                  # (frames that differ: Pillow's gif merges equal ones)
        return (torch.arange(t, dtype=torch.uint8) * 40).view(1, t, 1, 1, 1).expand(b, t, h, w, 3).contiguous().as_subclass(_OnDevice)

    def file(self, savetype, path, n, fps):
        """What the real container writes around the fixed bytes."""
        if savetype == "gif":
            return open(gif.write_gif(path, [(self.PALETTE, self.LZW)] * n, int(round(1000.0 / fps)), WA, H), "rb").read()
        if savetype == "png":
            return open(png.write_apng(path, [self.ZLIB] * n, int(round(1000.0 / fps)), WA, H), "rb").read()
        return open(mjpeg.write_avi(path, [self.JPEG] * n, fps, H, WA), "rb").read()


WRITERS = [("gif", "pillow", "gif", ".gif"), ("gif", "device", "gif", ".gif"), ("mjpeg", "pillow", "mjpeg", ".avi"), ("png", "pillow", "png", ".png")]


@pytest.mark.parametrize("savetype,gif_encoder,folder,ext", WRITERS)
@pytest.mark.parametrize("gpu_io", [False, True])
def test_perform_save_locally_video_names_numbers_and_hands_over_as_before(tmp_path, monkeypatch, savetype, gif_encoder, folder, ext, gpu_io):
    enc = _Encoders(monkeypatch)
    out, T, fps = str(tmp_path / "out"), 3, 5
    x = torch.rand(2, 3, T, H, WA, generator=torch.Generator().manual_seed(3))
    options = dict(gif_encoder=gif_encoder) if gif_encoder == "device" else {}
    if savetype == "mjpeg":
        options["video_quality"] = 77
    if gpu_io:
        x = (x * 2 - 1).as_subclass(_OnDevice)
        options.update(gpu_io=True, signed=True)
    on_device = savetype != "gif" or gif_encoder == "device"
    want_call = (("gif" if savetype == "gif" else savetype), (T, H, WA, 3)) + ((77,) if savetype == "mjpeg" else ())
    first = U.perform_save_locally_video(out, x, fps, savetype, return_savepaths=True, **options)
    assert first == [os.path.join(out, folder, f"animation-{i:04}{ext}") for i in (0, 1)]
    calls = enc.take()
    if gpu_io:
        assert calls[:2] == [("frames_to_u8", False, False), ("frames_to_u8", True, False)]      # the movie truncates, the grid rounds
        calls = calls[2:]
    assert calls == ([want_call] * 2 if on_device else [])
    assert sorted(os.listdir(os.path.join(out, "grid"))) == ["grid-0000.png", "grid-0001.png"]
    assert np.array(Image.open(os.path.join(out, "grid", "grid-0001.png"))).shape == (H, T * WA, 3)
    assert U.perform_save_locally_video(out, x[:1], fps, savetype, save_grid=False, **options) is None
    second = U.perform_save_locally_video(out, x[:1], fps, savetype, return_savepaths=True, save_grid=False, **options)
    assert second == [os.path.join(out, folder, f"animation-0003{ext}")]
    assert sorted(os.listdir(out)) == sorted({folder, "grid"}) and len(os.listdir(os.path.join(out, folder))) == 4
    assert len(os.listdir(os.path.join(out, "grid"))) == 2
    if on_device:
        assert open(second[0], "rb").read() == enc.file(savetype, str(tmp_path / "want"), T, fps)
    else:
        im = Image.open(first[1])
        assert im.n_frames == T and im.info["duration"] == 200 and im.size == (WA, H)
        if not gpu_io:                             # the movie's bytes are uint8(255 x), not the grid's uint8(255 x + 0.5)
            u8 = (255.0 * x[1].permute(1, 2, 3, 0).numpy()).astype(np.uint8)
            imgs, want = [Image.fromarray(f) for f in u8], io.BytesIO()
            imgs[0].save(want, "GIF", save_all=True, append_images=imgs[1:], duration=200, loop=0)
            assert open(first[1], "rb").read() == want.getvalue()
            grid = np.array(Image.open(os.path.join(out, "grid", "grid-0001.png")))
            assert np.array_equal(grid, np.concatenate(list(np.clip(x[1].permute(1, 2, 3, 0).numpy() * 255.0 + 0.5, 0, 255).astype(np.uint8)), axis=1))


def test_perform_save_locally_video_checks_in_the_same_order_with_the_same_words(tmp_path, monkeypatch):
    _Encoders(monkeypatch)
    x, out = torch.zeros(1, 3, 2, H, WA), str(tmp_path)
    with pytest.raises(AssertionError, match="Expected samples to have shape"):
        U.perform_save_locally_video(out, x[0], 4, "bmp", gif_encoder="gpu")
    with pytest.raises(AssertionError):
        U.perform_save_locally_video(out, x, 4, "bmp", gif_encoder="gpu")
    with pytest.raises(ValueError) as e:
        U.perform_save_locally_video(out, x, 4, "mp4", gif_encoder="gpu", signed=True)
    assert str(e.value) == "gif_encoder 'gpu': one of ('pillow', 'device')"
    with pytest.raises(ValueError) as e:
        U.perform_save_locally_video(out, x, 4, "mp4", gif_encoder="device", signed=True)
    assert str(e.value) == "gif_encoder='device' encodes gifs: savetype must be 'gif', got 'mp4'"
    with pytest.raises(AssertionError, match="signed samples are only taken on the gpu_io route"):
        U.perform_save_locally_video(out, x, 4, "mp4", signed=True)
    with pytest.raises(NotImplementedError, match="mp4 encoding needs imageio-ffmpeg / cv2"):
        U.perform_save_locally_video(out, x, 4, "mp4", gpu_io=True)
    for savetype, samples in (("npy", x.as_subclass(_OnDevice)), ("gif", x)):
        with pytest.raises(ValueError) as e:
            U.perform_save_locally_video(out, samples, 4, savetype, gpu_io=True)
        assert str(e.value) == "gpu_io saves uint8 frames (savetype='gif') of a device tensor"
    assert os.listdir(out) == []
    assert U.perform_save_locally_video(out, x, 4, "npy", return_savepaths=True) == [os.path.join(out, "npy", "frames-0000.npy")]
    assert U.perform_save_locally_video(out, torch.cat([x, x]), 4, "npy", return_savepaths=True) == [
        os.path.join(out, "npy", f"frames-{i:04}.npy") for i in (1, 2)]
    assert np.load(os.path.join(out, "npy", "frames-0002.npy")).shape == (2, H, WA, 3) and os.listdir(out) == ["npy"]
    assert U.GIF_ENCODERS == ("pillow", "device")


def test_the_save_functions_number_and_hand_over_alike(tmp_path, monkeypatch):
    enc = _Encoders(monkeypatch)
    out, fps = str(tmp_path / "out"), 7
    u8 = np.stack([_frame(i, H, WA) for i in range(3)])
    dev = torch.from_numpy(u8.copy())                                                    # (stands for a device tensor)
    saves = [("gif", ".gif", lambda f: U.save_gif_u8(out, f, fps, gif_encoder="device"), ("gif", (3, H, WA, 3))),
             ("mjpeg", ".avi", lambda f: U.save_avi_u8(out, f, fps, 55), ("mjpeg", (3, H, WA, 3), 55)),
             ("png", ".png", lambda f: U.save_png_u8(out, f, fps), ("png", (3, H, WA, 3)))]
    for folder, ext, save, call in saves:
        assert save(u8) == os.path.join(out, folder, f"animation-0000{ext}")           # a host array: uploaded once
        assert save(dev) == os.path.join(out, folder, f"animation-0001{ext}")
        assert enc.take() == [call, call]
        want = enc.file(folder, str(tmp_path / "want"), 3, fps)
        assert all(open(os.path.join(out, folder, f"animation-000{i}{ext}"), "rb").read() == want for i in (0, 1))
    assert U.save_avi_u8(out, u8, fps) == os.path.join(out, "mjpeg", "animation-0002.avi") and enc.take() == [("mjpeg", (3, H, WA, 3), 90)]
    # Pillow's gif: numbered in the same folder as the device's, written by the plain Pillow call
    path = U.save_gif_u8(out, u8, fps)
    assert path == os.path.join(out, "gif", "animation-0002.gif") and enc.take() == []
    imgs, want = [Image.fromarray(f) for f in u8], io.BytesIO()
    imgs[0].save(want, "GIF", save_all=True, append_images=imgs[1:], duration=int(round(1000.0 / fps)), loop=0)
    assert open(path, "rb").read() == want.getvalue()
    with pytest.raises(ValueError) as e:
        U.save_gif_u8(str(tmp_path / "none"), u8, fps, gif_encoder="gpu")
    assert str(e.value) == "gif_encoder 'gpu': one of ('pillow', 'device')" and not os.path.exists(str(tmp_path / "none"))


@pytest.mark.parametrize("savetype,gif_encoder,folder,ext", WRITERS)
def test_propagate_chunk_writes_result_full_through_the_same_writers(src, tmp_path, monkeypatch, savetype, gif_encoder, folder, ext):
    """--propagate: the Pillow gif goes through util.save_gif_u8 as it is found on the module at call time, with (path, host frames, fps);
    the device writers take the frames where they are."""
    import ccedit_amd.propagate
    enc = _Encoders(monkeypatch)
    out = str(tmp_path / "job")
    args = types.SimpleNamespace(H=H, W=WA, inpainting_mode=False, mask_composite=False, original_fps=6, target_fps=3, num_keyframes=3,
                                 save_type=savetype, video_quality=66, gif_encoder=gif_encoder)
    source = torch.from_numpy(np.stack([_frame(i, H, WA) for i in range(6)]))
    monkeypatch.setattr(U, "load_video_frames_u8", lambda path, size, device: source)
    monkeypatch.setattr(ccedit_amd.propagate, "propagate_clip", lambda source, idx, edited, masks=None: source)
    caught = []
    real_save = U.save_gif_u8
    if (savetype, gif_encoder) == ("gif", "pillow"):
        monkeypatch.setattr(U, "save_gif_u8", lambda path, frames, fps: (caught.append((path, frames, fps)), real_save(path, frames, fps))[1])
    samples = torch.zeros(2, 3, 3, H, WA)
    paths = S.propagate_chunk(args, [src.path("clip.avi"), src.path("clip.avi")], samples, CPU, out)
    assert paths == [os.path.join(out, "result_full", folder, f"animation-{i:04}{ext}") for i in (0, 1)]
    assert all(os.path.isfile(p) for p in paths) and os.listdir(out) == ["result_full"] and os.listdir(os.path.join(out, "result_full")) == [folder]
    calls = enc.take()
    assert calls[0] == ("frames_to_u8", False, False)
    if (savetype, gif_encoder) == ("gif", "pillow"):
        assert calls[1:] == [] and len(caught) == 2
        for path, frames, fps in caught:
            assert path == os.path.join(out, "result_full") and type(frames) is np.ndarray and np.array_equal(frames, source.numpy()) and fps == 6
        assert Image.open(paths[1]).info["duration"] == int(round(1000.0 / 6) // 10 * 10)
    else:
        assert caught == [] and calls[1:] == [(folder, (6, H, WA, 3)) + ((66,) if savetype == "mjpeg" else ())] * 2
        assert open(paths[1], "rb").read() == enc.file(savetype, str(tmp_path / "want"), 6, 6)


@pytest.mark.parametrize("savetype,gif_encoder,folder,ext", WRITERS + [("npy", "pillow", None, None)])
@pytest.mark.parametrize("gpu_io", [False, True])
def test_save_result_hands_the_options_of_the_arguments_to_the_one_writer(tmp_path, monkeypatch, savetype, gif_encoder, folder, ext, gpu_io):
    enc = _Encoders(monkeypatch)
    out = str(tmp_path / "single")
    args = types.SimpleNamespace(save_path=out, save_type=savetype, video_quality=66, gif_encoder=gif_encoder, gpu_io=gpu_io, target_fps=4)
    x = torch.rand(1, 3, 2, H, WA, generator=torch.Generator().manual_seed(5)) * 2 - 1
    S.save_result(args, "tag", x.as_subclass(_OnDevice) if gpu_io else x)
    calls = enc.take()
    if folder is None:                                                                        # (.npy: save_frames alone, as ever)
        assert calls == [] and os.listdir(os.path.join(out, "result")) == ["tag.npy"]
        return
    assert sorted(os.listdir(os.path.join(out, "result"))) == sorted([folder, "grid", "tag.npy"])
    assert os.listdir(os.path.join(out, "result", folder)) == [f"animation-0000{ext}"] and os.listdir(os.path.join(out, "result", "grid")) == ["grid-0000.png"]
    if gpu_io:
        assert calls[:2] == [("frames_to_u8", False, False), ("frames_to_u8", True, False)]      # signed: clamp((x + 1) / 2) is the kernel's
        calls = calls[2:]
    if (savetype, gif_encoder) == ("gif", "pillow"):
        assert calls == [] and Image.open(os.path.join(out, "result", "gif", "animation-0000.gif")).info["duration"] == 250
    else:
        assert calls == [(folder, (2, H, WA, 3)) + ((66,) if savetype == "mjpeg" else ())]
        assert open(os.path.join(out, "result", folder, f"animation-0000{ext}"), "rb").read() == enc.file(savetype, str(tmp_path / "want"), 2, 4)
