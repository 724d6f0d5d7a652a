"""Pixel I/O on the GPU, the parts that can be checked without one: the six C-ABI entry points are declared, exported, bound and
validate their arguments before any HIP call; the host-built tap tables of the 8-bit resize, applied by a plain integer numpy
loop, reproduce Pillow's Image.resize(BICUBIC) bit for bit (csrc/pixel.hip applies the same tables)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PIXEL_SYMBOLS = ("ccedit_resize_u8_pil", "ccedit_resize_f32_bicubic", "ccedit_kth_values", "ccedit_minmax_f32", "ccedit_depth_hint",
                 "ccedit_frames_to_u8")


@pytest.fixture(scope="module")
def lib():
    from ccedit_amd.csrc.build import build
    build(force=False, verbose=False)
    from ccedit_amd import hip
    return hip.lib()


def _frames(n=23, h=40, w=56):           # == tests/test_video_io.py::_frames (the frames the goldens were recorded from)
    rs = np.random.RandomState(5)
    yy, xx = np.mgrid[0:h, 0:w]
    return [np.stack([(xx * 4 + 7 * i) % 256, (yy * 5 + 3 * i) % 256, rs.randint(0, 256, (h, w))], -1).astype(np.uint8)
            for i in range(n)]


def test_pixel_symbols_declared_exported_and_bound(lib):
    from ccedit_amd import hip, ops, packing
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ccedit_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(hip.LIB_PATH)
    for name in PIXEL_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/ccedit_hip.h"
        assert hasattr(raw, name), f"{name} is not exported by the library"
        assert name in hip.EXPORTS
    for name in ("resize_u8_pil", "resize_bicubic", "kth_values", "minmax", "depth_hint", "frames_to_u8"):
        assert callable(getattr(ops, name))
    assert callable(packing.pil_bicubic_taps) and callable(packing.aten_bicubic_taps)
    assert lib.ccedit_abi_version() == 12          # additive: the ABI version does not move


def test_pixel_entry_points_validate_before_any_hip_call(lib):
    """Null pointers and impossible sizes: negative code + message, no launch (there is no GPU here)."""
    P = 64          # any non-null "pointer": nothing is dereferenced before the checks fail

    def err():
        return lib.ccedit_last_error()
    assert lib.ccedit_resize_u8_pil(None, P, P, P, 4, P, 4, 1, 8, 8, 4, 4, 0, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_resize_u8_pil(P, P, P, None, 4, P, 4, 1, 8, 8, 4, 4, 0, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_resize_u8_pil(P, P, P, P, 4, P, 4, 0, 8, 8, 4, 4, 0, None) == -1 and b"positive" in err()
    assert lib.ccedit_resize_u8_pil(P, P, P, P, 4, P, 4, 1, 8, -8, 4, 4, 0, None) == -1 and b"positive" in err()
    assert lib.ccedit_resize_u8_pil(P, P, P, P, 0, P, 4, 1, 8, 8, 4, 4, 0, None) == -1 and b"tap counts" in err()
    assert lib.ccedit_resize_u8_pil(P, P, P, P, 4, None, 0, 1, 8, 8, 4, 4, 0, None) == -1 and b"xtab" in err()       # width changes: needs xtab
    assert lib.ccedit_resize_u8_pil(P, P, None, P, 4, P, 4, 1, 8, 8, 4, 4, 0, None) == -1 and b"tmp" in err()
    assert lib.ccedit_resize_u8_pil(P, P, P, P, 4, P, 4, 1 << 20, 1 << 10, 1 << 10, 4, 4, 0, None) == -1 and b"2^31" in err()
    assert lib.ccedit_resize_f32_bicubic(None, P, P, P, 3, 8, 8, 4, 4, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_resize_f32_bicubic(P, P, P, None, 3, 8, 8, 4, 4, None) == -1
    assert lib.ccedit_resize_f32_bicubic(P, P, P, P, 0, 8, 8, 4, 4, None) == -1 and b"positive" in err()
    assert lib.ccedit_resize_f32_bicubic(P, P, P, P, 3, 8, 8, 0, 4, None) == -1
    ranks = (ctypes.c_int64 * 2)(1, 5)
    assert lib.ccedit_kth_values(None, 1, 10, ranks, 2, P, P, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_kth_values(P, 1, 10, None, 2, P, P, None) == -1
    assert lib.ccedit_kth_values(P, 1, 10, ranks, 2, P, None, None) == -1
    assert lib.ccedit_kth_values(P, 0, 10, ranks, 2, P, P, None) == -1 and b"B=0" in err()
    assert lib.ccedit_kth_values(P, 1, 1 << 31, ranks, 2, P, P, None) == -1
    assert lib.ccedit_kth_values(P, 1, 10, ranks, 5, P, P, None) == -1 and b"n_ranks" in err()
    assert lib.ccedit_kth_values(P, 1, 4, ranks, 2, P, P, None) == -1 and b"rank 5 outside" in err()
    assert lib.ccedit_kth_values(P, 1, 10, (ctypes.c_int64 * 1)(0), 1, P, P, None) == -1 and b"rank 0 outside" in err()
    assert lib.ccedit_minmax_f32(None, 1, 10, P, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_minmax_f32(P, 1, 0, P, None) == -1
    assert lib.ccedit_minmax_f32(P, 70000, 10, P, None) == -1
    assert lib.ccedit_depth_hint(P, P, None, 0, 1, 10, 1, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_depth_hint(P, P, P, 1, 1, 10, 1, None) == -1 and b"stat_stride" in err()
    assert lib.ccedit_depth_hint(P, P, P, 0, 1, 0, 1, None) == -1
    assert lib.ccedit_frames_to_u8(P, None, 1, 10, 0, 0, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_frames_to_u8(P, P, 1, 10, 2, 0, None) == -1 and b"mode=2" in err()
    assert lib.ccedit_frames_to_u8(P, P, 0, 10, 0, 0, None) == -1


def _pil_resize(img, h, w):
    from PIL import Image
    return np.array(Image.fromarray(img).resize((w, h), Image.BICUBIC))


@pytest.mark.parametrize("hs,ws,h,w", [(270, 480, 128, 192),      # shrink (antialiased: up to 11 taps)
                                       (64, 96, 128, 192),        # enlargement
                                       (40, 56, 40, 30),          # height unchanged
                                       (37, 53, 61, 53),          # width unchanged
                                       (101, 67, 33, 97)])        # one axis shrinks, the other grows; odd sizes
def test_tap_tables_reproduce_pillow_bit_for_bit(hs, ws, h, w):
    from ccedit_amd.packing import apply_pil_taps_reference, pil_bicubic_taps
    img = np.random.RandomState(hs + w).randint(0, 256, (hs, ws, 3)).astype(np.uint8)
    img[: hs // 3, : ws // 2] = np.where(img[: hs // 3, : ws // 2] > 127, 255, 0)          # hard edges: overshoot is clipped to 0 ... 255
    ytab, xtab = pil_bicubic_taps(hs, h), pil_bicubic_taps(ws, w)
    for tab, size in ((ytab, hs), (xtab, ws)):
        assert tab.dtype == np.int32 and (tab[:, 0] >= 0).all() and (tab[:, 0] + tab[:, 1] <= size).all() and (tab[:, 1] <= tab.shape[1] - 2).all()
        assert np.abs(tab[:, 2:].astype(np.int64)).sum(axis=1).max() < 1.4 * (1 << 22)          # 255 * sum|w| + 2^21 fits int32
    assert np.array_equal(apply_pil_taps_reference(img, ytab, xtab), _pil_resize(img, h, w))


def test_tap_tables_reproduce_the_reference_goldens(golden_dir):
    """The two resized goldens of tests/golden/video_io.npz were recorded from the reference's load_img / load_video_keyframes
    (Pillow resize, / 255, * 2 - 1): the tables + integer loop give the same floats."""
    from ccedit_amd.packing import apply_pil_taps_reference, pil_bicubic_taps
    from scripts.sampling.util import keyframe_indices
    z = np.load(os.path.join(golden_dir, "video_io.npz"))
    fr = _frames()

    def as_float(u8):          # (.., H, W, 3) uint8 -> (.., 3, H, W) as load_img does
        t = torch.from_numpy(u8).movedim(-1, -3).float() / 255.0
        return torch.clamp(t * 2.0 - 1.0, -1.0, 1.0).numpy()
    got = apply_pil_taps_reference(fr[3], pil_bicubic_taps(40, 24), pil_bicubic_taps(56, 40))
    assert np.array_equal(as_float(got)[None], z["img_resized"])
    clip = np.stack([fr[i] for i in keyframe_indices(23, 20, 3, 5)])
    got = apply_pil_taps_reference(clip, pil_bicubic_taps(40, 32), pil_bicubic_taps(56, 48))
    assert np.array_equal(as_float(got), z["dir_20_3_5_resized"])


def test_aten_tap_tables_match_interpolate():
    """The fp32 tables of ccedit_resize_f32_bicubic (four taps, a = -0.75, border clamp) applied in numpy agree with
    F.interpolate(mode="bicubic", align_corners=False) to fp32 rounding (the GPU test holds the kernel to 1e-5)."""
    from ccedit_amd.packing import aten_bicubic_taps
    x = torch.rand(2, 3, 40, 56, generator=torch.Generator().manual_seed(0)) * 2 - 1

    def apply(src, tab, axis):
        src = np.moveaxis(src, axis, 0)
        wts = tab[:, 2:].view(np.float32)
        out = np.zeros((tab.shape[0],) + src.shape[1:], np.float32)
        for i in range(tab.shape[0]):
            for k in range(4):
                out[i] += wts[i, k] * src[min(max(tab[i, 0] + k, 0), src.shape[0] - 1)]
        return np.moveaxis(out, 0, axis)
    for h, w in ((32, 48), (80, 100), (40, 33)):
        ref = torch.nn.functional.interpolate(x, size=(h, w), mode="bicubic", align_corners=False).numpy()
        got = apply(apply(x.numpy(), aten_bicubic_taps(56, w), 3), aten_bicubic_taps(40, h), 2)
        assert np.abs(got - ref).max() < 1e-5
    x = torch.rand(1, 1, 48, 512, generator=torch.Generator().manual_seed(1)) * 2 - 1          # coordinates up to 512: the source position
    ref = torch.nn.functional.interpolate(x, size=(64, 768), mode="bicubic", align_corners=False).numpy()          # needs its single rounding
    got = apply(apply(x.numpy(), aten_bicubic_taps(512, 768), 3), aten_bicubic_taps(48, 64), 2)
    assert np.abs(got - ref).max() < 1e-5


def test_host_routes_keep_their_signatures_and_the_flag_is_off_by_default():
    import argparse
    import inspect
    from scripts.sampling import util
    from scripts.sampling.sampling_tv2v import add_common_args
    from sgm.modules.encoders.modules import DepthMidasEncoder, DepthZoeEncoder
    for fn in (util.load_img, util.load_video_keyframes):
        assert inspect.signature(fn).parameters["device"].default is None
    sig = inspect.signature(util.perform_save_locally_video).parameters
    assert sig["gpu_io"].default is False and sig["signed"].default is False
    p = argparse.ArgumentParser()
    add_common_args(p)
    assert p.parse_args([]).gpu_io is False and p.parse_args(["--gpu_io"]).gpu_io is True
    for cls in (DepthMidasEncoder, DepthZoeEncoder):
        assert callable(cls.normalize_gpu) and cls.normalize_gpu is not cls.normalize
    with pytest.raises(AssertionError):          # signed samples belong to the device route only
        util.perform_save_locally_video("unused", torch.zeros(1, 3, 1, 2, 2), fps=1, signed=True)


def test_pixel_object_has_no_packed_shift_saturate(lib):
    """csrc/pixel.hip: clip8.  v_ashr_pk_u8_i32 left stale bits in the high half of its destination on the MI355X (every packed word
    after the first had a wrong byte 2); the kernels are written so that the compiler does not select it."""
    import shutil
    import subprocess
    import tempfile
    from ccedit_amd.csrc import build
    obj = os.path.join(build.HERE, "pixel.o")
    if not (os.path.exists(build.OBJDUMP) and os.path.exists(obj)):
        pytest.skip("llvm-objdump or the object file not present")
    with tempfile.TemporaryDirectory() as tmp:
        o = shutil.copy(obj, tmp)
        subprocess.run([build.OBJDUMP, "--offloading", o], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=False)
        dis = "".join(subprocess.run([build.OBJDUMP, "-d", os.path.join(tmp, f)], capture_output=True, text=True, check=False).stdout
                      for f in os.listdir(tmp) if "amdgcn" in f)
    assert "global_store" in dis and "v_ashr_pk_u8_i32" not in dis
