"""GIF sources decoded on the device, everything that needs no device (ccedit_amd/gifdec.py, csrc/gifdec_core.h):
the numpy restatement of the three stages against a classic dictionary decoder and against Pillow, byte for byte, on every served case
of tests/_gifdec_cases.py; the parser's refusals; the statuses of broken streams; csrc/gifdec_core.h itself, compiled for the host with
the sanitizers, on every case stream and on 2000 seeded corruptions; the opt-in route of the loaders with a recorder in the place of the
device; the command line's check."""
import io
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gifdec_cases as K  # noqa: E402
import _gifdec_numpy as R  # noqa: E402
from ccedit_amd import gifdec, ops, video_io  # noqa: E402
from scripts.sampling import sampling_tv2v as S  # noqa: E402
from scripts.sampling import sampling_tv2v_ref as SR  # noqa: E402
from scripts.sampling import util as U  # noqa: E402

CPU = torch.device("cpu")
TAIL = "; this clip is decoded by Pillow on the host\n"


# ---- 1. the formulation ---------------------------------------------------------------------------
def test_the_cases_cover_what_they_are_named_for():
    """The mechanisms are really in the streams: full tables, widths up to 12, strings above 256, every code a KwKwK, the code counts
    at the batch edges, the sub-block lengths."""
    def table(name, frame=0):
        return K.expected(name)[2][frame]

    def stream(name):
        f = K.expected(name)[0].frames[0]
        return f.stream

    assert len(table("noise-deferred-clear")[0]) > 4096 - 258 + 64 and len(table("noise-m2-table-fills")[0]) > 4096
    assert int(table("flat-256x256")[1].max()) > 256
    parent = table("flat-48x72")[0]
    assert np.array_equal(parent[1:-1], np.arange(len(parent) - 2))                 # every code (but the remainder) names the entry it completes itself
    for n in (1, 2, 63, 64, 65):
        assert len(table(f"codes-{n}")[0]) == n
    assert len(table("eoi-as-64th-code")[0]) == 63
    assert [len(stream(f"stream-{n}-bytes")) for n in (254, 255, 256, 510)] == [254, 255, 256, 510]
    assert {K.expected(f"m{m}-noise")[0].frames[0].min_code for m in range(2, 9)} == set(range(2, 9))
    for name in K.all_served():
        for f in K.expected(name)[0].frames:
            assert f.h <= 256 and f.w <= 256


def test_the_width_rule_is_the_classic_decoders():
    """width_at (the count of codes since the Clear alone) against the classic bookkeeping: next free entry, one bit more when it
    reaches 2^width."""
    for m in range(2, 9):
        nxt, width = (1 << m) + 2, m + 1
        for j in range(5000):
            assert R.width_at(m, j) == width, (m, j)
            if j >= 1 and nxt < 4096:                     # (the first code after a Clear makes no entry)
                nxt += 1
                if nxt == (1 << width) and width < 12:
                    width += 1


@pytest.mark.parametrize("name", sorted(K.all_served()))
def test_reference_equals_the_classic_decoder_and_pillow(name):
    info, want, tables, planes = K.expected(name)
    for f, plane in zip(info.frames, planes):
        classic = R.classic_indices(f.stream, f.min_code, f.w * f.h)
        assert classic is not None and bytes(plane) == classic
    got = R.decode(info)
    assert got.shape == want.shape and got.dtype == np.uint8 and np.array_equal(got, want)


# ---- 2. the parser --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.declined()))
def test_declined_files_name_their_reason_and_stay_pillows(name):
    data, reason = K.declined()[name]
    with pytest.raises(gifdec.GifUnsupported) as e:
        gifdec.parse(data)
    assert reason in str(e.value)
    assert Image.open(io.BytesIO(data)).format == "GIF"


def test_structural_defects_are_value_errors():
    good = K.served()["1x1"]
    for data, text in ((b"GIF88a" + good[6:], "bad signature"), (good[:-1] + b"\x07", "unknown block 0x07"), (b"", "bad signature")):
        with pytest.raises(ValueError) as e:
            gifdec.parse(data)
        assert text in str(e.value) and not isinstance(e.value, gifdec.GifUnsupported)
    for cut in range(6, len(good) - 1):
        with pytest.raises(gifdec.GifUnsupported) as e:
            gifdec.parse(good[:cut])
        assert "truncated file" in str(e.value)


def test_parse_reads_descriptors_palettes_and_sub_blocks():
    info = gifdec.parse(K.served()["transparent-local-palette"])
    assert (info.height, info.width, info.n_frames) == (30, 40, 3)
    f = info.frames[1]
    assert (f.x, f.y, f.w, f.h, f.transparent, f.min_code, len(f.palette), f.interlace, f.disposal) == (3, 4, 25, 20, 5, 4, 48, False, 0)
    assert info.frames[0].transparent == -1 and len(info.frames[0].palette) == 768
    assert gifdec.parse(K.served()["interlaced-9-rows"]).frames[1].interlace
    assert gifdec.parse(K.served()["disposal-2-on-the-last-frame"]).frames[-1].disposal == 2
    f = gifdec.parse(K.served()["stream-510-bytes"]).frames[0]
    assert len(f.stream) == 510 and f.max_codes == min(16 * 14, 8 * 510 // 9) + 1
    data, desc, codes, plane, largest = gifdec.describe(info.frames, [0, -1, 1])
    assert desc.shape == (3, gifdec.DESC_WORDS) and codes == sum(f.max_codes for f in info.frames) and plane == 30 * 40 * 2 + 25 * 20
    assert largest == max(f.max_codes for f in info.frames) and list(desc[:, gifdec.D_SLOT]) == [0, -1, 1]
    assert desc[1, gifdec.D_PAL_OFF] == desc[2, gifdec.D_PAL_OFF] and desc[1, gifdec.D_PAL_SIZE] == 16       # (one copy of a shared palette)
    for i, f in enumerate(info.frames):
        lo, n = int(desc[i, gifdec.D_STREAM_OFF]), int(desc[i, gifdec.D_STREAM_LEN])
        assert bytes(data[lo:lo + n]) == f.stream
        lo = int(desc[i, gifdec.D_PAL_OFF])
        assert bytes(data[lo:lo + len(f.palette)]) == f.palette


# ---- 3. statuses -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.stopped()))
def test_stopped_streams_give_their_status_in_the_reference(name):
    data, status, frame = K.stopped()[name]
    info = gifdec.parse(data)
    with pytest.raises(ValueError) as e:
        R.decode(info)
    assert str(e.value).startswith(f"frame {frame}: status {status}")
    assert Image.open(io.BytesIO(data)).format == "GIF"


def test_status_texts():
    assert set(gifdec.STATUS_TEXT) == {1, 2, 3, 4, 5, 6}
    assert str(gifdec.status_error(1, 27, 4)) == "frame 4: a code above the next free entry (code 1 at bit 27)"
    assert str(gifdec.status_error(5, 9, 0)) == "frame 0: an index at or beyond the palette's size (code 5 at pixel 9)"


# ---- 4. the core under the host's sanitizers ------------------------------------------------------
def test_the_core_on_the_host_under_the_sanitizers():
    """Every case stream by one lane and by 64 emulated lanes in descending order: the same tables, statuses and positions, the
    reference's indices; then 2000 seeded corruptions: a defined status each — the reference's —, no sanitizer report."""
    cases, want = [], []
    for name, m, npix, stream in K.case_streams():
        t = R.code_table(stream, m, npix)
        cases.append((m, npix, stream, R.classic_indices(stream, m, npix)))
        want.append((t[5], t[6], len(t[0])))
    n_valid = sum(c[3] is not None for c in cases)
    assert n_valid >= 60 and len(cases) - n_valid == 4                                   # (the stopped streams, but the bad index: a stage C status)
    for name, m, npix, stream in K.corruptions():
        t = R.code_table(stream, m, npix)
        cases.append((m, npix, stream, None))
        want.append((t[5], t[6], len(t[0])))
    assert len(cases) - len(K.case_streams()) == 2000
    got = K.run_host_core(cases)
    assert [tuple(int(v) for v in row) for row in got] == want
    assert {w[0] for w in want[len(K.case_streams()):]} >= {0, 1, 2, 3}                   # (the corruptions reach every stream status)
    # the defence statuses, and a table with no room
    extra = K.run_host_core([(1, 4, b"\x00", None), (9, 4, b"\x00", None), (8, 4, b"", None)])
    assert [tuple(int(v) for v in row) for row in extra] == [(4, 0, 0), (4, 0, 0), (3, 0, 0)]


# ---- 5. the routes --------------------------------------------------------------------------------
class _Recorder:
    """Stands in for the device decoder and the ops functions of the loaders; `calls` is what ran, in order."""

    def __init__(self, monkeypatch):
        self.calls = []
        self.fail = None
        monkeypatch.setattr(gifdec, "decode_gif", self._decode_gif)
        monkeypatch.setattr(ops, "resize_u8_pil", self._resize_u8_pil)
        monkeypatch.setattr(ops, "resize_bicubic", self._resize_bicubic)
        monkeypatch.setattr(ops, "frames_to_u8", self._frames_to_u8)

    def take(self):
        out, self.calls = self.calls, []
        return out

    def _decode_gif(self, data, device, select=None, info=None, frames_per_group=None):
        assert device == CPU and info is not None and frames_per_group is None             # (the file was parsed once, by the router)
        idx = list(range(info.n_frames)) if select is None else [int(i) for i in select(info.n_frames)]
        self.calls.append(("gifdec.decode_gif", bytes(data), tuple(idx)))
        if self.fail is not None:
            raise self.fail
        return torch.zeros((len(idx), info.height, info.width, 3), dtype=torch.uint8)

    def _resize_u8_pil(self, x, size, to_float=False):
        self.calls.append(("resize_u8_pil", tuple(x.shape), tuple(int(v) for v in size), bool(to_float)))
        return torch.zeros((3, x.shape[0], size[0], size[1])) if to_float else torch.zeros((x.shape[0], size[0], size[1], 3), dtype=torch.uint8)

    def _resize_bicubic(self, x, size):
        self.calls.append(("resize_bicubic", tuple(x.shape), tuple(size)))
        return torch.zeros((x.shape[0], x.shape[1], size[0], size[1]))

    def _frames_to_u8(self, x, rounding=False, unit_range=False):
        self.calls.append(("frames_to_u8", tuple(x.shape), bool(rounding), bool(unit_range)))
        b, _, t, h, w = x.shape
        return torch.zeros((b, t, h, w, 3), dtype=torch.uint8)


@pytest.fixture
def rec(monkeypatch):
    return _Recorder(monkeypatch)


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    root = tmp_path_factory.mktemp("gifdec_routes")
    out = {}
    for name, data in (("served", K.served()["rectangles-at-the-corners"]), ("declined", K.declined()["disposal-2-in-mid-clip"][0])):
        out[name] = str(root / f"{name}.gif")
        with open(out[name], "wb") as f:
            f.write(data)
    return out


def test_the_table_keeps_the_default_route_and_names_the_opt_in():
    assert video_io.GIF.device == () and video_io.GIF.opt_in == (video_io.GIFDEC,)
    assert all(k.opt_in == () for k in video_io.KINDS if k is not video_io.GIF)
    assert video_io.GIFDEC.module is gifdec and video_io.GIFDEC.declines is ValueError and video_io.GIFDEC.ext == ()
    assert video_io.decoders_of(video_io.GIF) == () and video_io.decoders_of(video_io.GIF, "pillow") == ()
    assert video_io.decoders_of(video_io.GIF, "device") == (video_io.GIFDEC,) and video_io.decoders_of(video_io.GIF, "gpu") == ()
    assert video_io.decoders_of(video_io.APNG, "device") == (video_io.PNG,) and video_io.decoders_of(video_io.FILES, "device") == video_io.FILES.device


def test_by_default_a_gif_is_pillows(clips, rec, capsys):
    path = clips["served"]                                                                # 6 frames of 30 x 40
    for extra in ({}, {"gif_decoder": "pillow"}):
        x = U.load_video_keyframes(path, 6, 3, 3, size=(8, 12), device=CPU, **extra)
        assert rec.take() == [("resize_u8_pil", (3, 30, 40, 3), (30, 40), True), ("resize_bicubic", (3, 3, 30, 40), (8, 12))] and x.shape == (3, 3, 8, 12)
        x = U.load_video_frames_u8(path, (8, 12), CPU, **extra)
        assert [c[0] for c in rec.take()] == ["resize_u8_pil", "resize_bicubic", "frames_to_u8"] and x.shape == (6, 8, 12, 3)
    assert U.load_video_keyframes(path, 6, 3, 3, gif_decoder="device").shape == (3, 3, 30, 40)       # (no device: the host route)
    assert rec.take() == [] and capsys.readouterr().err == ""


def test_with_the_device_decoder_the_selected_frames_are_decoded_there(clips, rec, capsys):
    path = clips["served"]
    data = open(path, "rb").read()
    x = U.load_video_keyframes(path, 6, 3, 3, size=(8, 12), device=CPU, gif_decoder="device")
    assert rec.take() == [("gifdec.decode_gif", data, (0, 2, 4)), ("resize_u8_pil", (3, 30, 40, 3), (30, 40), True),
                          ("resize_bicubic", (3, 3, 30, 40), (8, 12))] and x.shape == (3, 3, 8, 12)
    x = U.load_video_frames_u8(path, (8, 12), CPU, gif_decoder="device")
    assert rec.take()[0] == ("gifdec.decode_gif", data, (0, 1, 2, 3, 4, 5)) and x.shape == (6, 8, 12, 3)
    assert capsys.readouterr().err == ""


def test_a_declined_file_goes_through_pillow_with_one_line(clips, rec, capsys):
    path = clips["declined"]
    x = U.load_video_keyframes(path, 3, 3, 3, device=CPU, gif_decoder="device")
    assert rec.take() == [("resize_u8_pil", (3, 30, 40, 3), (30, 40), True)] and x.shape == (3, 3, 30, 40)
    assert capsys.readouterr().err == f"[gifdec] {path}: frame 1: disposal 2 before the last frame (only 0 and 1)" + TAIL


def test_a_device_status_is_a_value_error_naming_path_and_frame(clips, rec, capsys):
    path = clips["served"]
    rec.fail = gifdec.status_error(3, 288, 2)
    with pytest.raises(ValueError) as e:
        U.load_video_keyframes(path, 6, 3, 3, device=CPU, gif_decoder="device")
    assert str(e.value) == f"{path}: frame 2: the stream ends before the image's pixels (code 3 at bit 288)"
    assert capsys.readouterr().err == ""


def test_masks_stay_pillows(clips, rec, capsys):
    m = U.load_video_mask(clips["served"], 6, 3, 3, num_allframes=6, device=CPU)
    assert m.shape == (3, 30, 40) and rec.take() == [] and capsys.readouterr().err == ""


# ---- 6. the command line --------------------------------------------------------------------------
@pytest.mark.parametrize("module", [S, SR])
def test_gif_decoder_device_needs_gpu_io(module, capsys):
    p = module.make_parser()
    args = p.parse_args(["--gif_decoder", "device", "--gpu_io"])
    S.check_args(p, args)
    assert args.gif_decoder == "device" and p.parse_args([]).gif_decoder == "pillow"
    with pytest.raises(SystemExit) as e:
        S.check_args(p, p.parse_args(["--gif_decoder", "device"]))
    assert e.value.code == 2 and "--gif_decoder device decodes .gif sources where --gpu_io keeps the frames: add --gpu_io" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        p.parse_args(["--gif_decoder", "gpu"])


def test_the_flag_reaches_the_video_loaders_through_the_device_dict(monkeypatch):
    import types
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    on = types.SimpleNamespace(gpu_io=True, gif_decoder="device")
    assert S._io_device(on, video=True) == {"device": torch.device("cuda", 0), "gif_decoder": "device"}
    assert S._io_device(on) == {"device": torch.device("cuda", 0)}                          # (images and masks)
    assert S._io_device(types.SimpleNamespace(gpu_io=True, gif_decoder="pillow"), video=True) == {"device": torch.device("cuda", 0)}
    assert S._io_device(types.SimpleNamespace(gpu_io=True), video=True) == {"device": torch.device("cuda", 0)}
    assert S._io_device(types.SimpleNamespace(gpu_io=False, gif_decoder="device"), video=True) == {}
