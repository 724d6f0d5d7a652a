"""Mask tracking (`--mask_track`), the parts that can be checked without a GPU: the properties of the numpy restatement
(tests/_masktrack_numpy.py) that make it worth matching — it follows a moving subject where a static mask does not, and the
forward-backward check earns its place —, the host logic of ccedit_amd/masktrack.py (constants, pair lists, refusals), the
command-line surface of both entry points, and the three C-ABI entry points: declared, exported, bound, arguments validated before
any HIP call.

The bounds are intersection over union of the tracked mask against the truth, minimum over the frames of the clip; the clips are the
scene() generator's object moving over a moving background."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _masktrack_numpy as ref  # noqa: E402
from _masktrack_scenes import scene  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ("ccedit_masktrack_select", "ccedit_masktrack_step", "ccedit_mask_dilate")

# (bg, obj, frames) at 128 x 192, bound 0.95; (bg, obj) at 64 x 64 with 7 frames (a 21-pixel object), bound 0.85
LARGE = [((1, -2), (-2, 3), 13), ((2, 1), (2, 1), 13), ((-1, 1), (3, -4), 9)]
SMALL = [((0, 0), (1, 2)), ((1, 0), (-1, 2))]


@functools.lru_cache(maxsize=None)
def _scene(h, w, frames, bg, obj, noise=0.0):
    return scene(h, w, frames, bg=bg, obj=obj, noise=noise)


@functools.lru_cache(maxsize=None)
def _track(h, w, frames, bg, obj, anchor, noise=0.0, limit=ref.FB_LIMIT):
    clip, truth = _scene(h, w, frames, bg, obj, noise)
    return ref.track(clip, truth[anchor], anchor, limit)


def _min_iou(h, w, frames, bg, obj, anchor, noise=0.0, limit=ref.FB_LIMIT):
    out = _track(h, w, frames, bg, obj, anchor, noise, limit)
    truth = _scene(h, w, frames, bg, obj, noise)[1]
    assert out.dtype == np.uint8 and set(np.unique(out)) <= {0, 255}, "masks stay binary"
    assert np.array_equal(out[anchor], truth[anchor])
    ious = [ref.iou(out[f], truth[f]) for f in range(frames)]
    print(f"{h}x{w} bg={bg} obj={obj} anchor={anchor} noise={noise} limit={limit}: min IoU {min(ious):.3f}")
    return min(ious)


# ---- 1. properties of the restatement ----------------------------------------------------------------
def test_zero_motion_keeps_the_anchor_mask_exactly():
    clip, truth = _scene(64, 64, 5, (0, 0), (0, 0))
    for anchor in (0, 2, 4):
        out = ref.track(clip, truth[anchor], anchor)
        for f in range(5):
            assert np.array_equal(out[f], truth[anchor])


@pytest.mark.parametrize("bg,obj,frames", LARGE)
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_tracks_at_128x192(bg, obj, frames, where):
    anchor = {"first": 0, "middle": frames // 2, "last": frames - 1}[where]
    assert _min_iou(128, 192, frames, bg, obj, anchor) >= 0.95


@pytest.mark.parametrize("bg,obj", SMALL)
def test_tracks_a_21_pixel_object_at_64x64(bg, obj):
    assert _scene(64, 64, 7, bg, obj)[1][0].sum() == 255 * 21 * 21
    assert _min_iou(64, 64, 7, bg, obj, 0) >= 0.85


@pytest.mark.parametrize("h,w,frames,bg,obj", [(128, 192, f, b, o) for b, o, f in LARGE] + [(64, 64, 7, b, o) for b, o in SMALL])
def test_a_static_mask_misses_the_subject(h, w, frames, bg, obj):
    """The anchor mask held still scores below 0.5 at the far frame: the bounds above would notice tracking that does nothing."""
    truth = _scene(h, w, frames, bg, obj)[1]
    assert ref.iou(truth[0], truth[frames - 1]) < 0.5


def test_the_forward_backward_check_earns_its_place():
    """Without it (the limit out of reach) revealed background keeps the mask it is looked up under: the mask trails behind the object."""
    bg, obj, frames = LARGE[1]
    assert _min_iou(128, 192, frames, bg, obj, 0, limit=10 ** 9) < 0.8
    assert _min_iou(128, 192, frames, bg, obj, 0) >= 0.95


@pytest.mark.parametrize("bg,obj,frames", LARGE)
def test_noise_keeps_the_bounds_at_128x192(bg, obj, frames):
    assert _min_iou(128, 192, frames, bg, obj, 0, noise=3.0) >= 0.95


@pytest.mark.parametrize("bg,obj", SMALL)
def test_noise_keeps_the_bounds_at_64x64(bg, obj):
    assert _min_iou(64, 64, 7, bg, obj, 0, noise=3.0) >= 0.85


def test_select_prefers_the_lower_order_on_ties_and_clamps_vectors():
    flat = np.full((64, 64), 90, np.uint8)
    vec = np.random.RandomState(0).randint(-5, 6, (8, 8, 2))
    sel = ref.select(flat, flat, vec)
    assert np.array_equal(sel, np.repeat(np.repeat(vec, 8, 0), 8, 1)), "every sum is 0: candidate (0, 0), the block's own vector"
    huge = ref.select(flat, flat, np.full((8, 8, 2), 10 ** 6))
    assert (huge == ref.VEC_MAX).all()


def test_dilate_and_invert():
    m = np.zeros((2, 16, 24), np.uint8)
    m[0, 0, 0] = m[1, 8, 23] = 255
    d = ref.dilate(m, 2)
    assert d[0, :3, :3].all() and d[0].sum() == 255 * 9 and d[1, 6:11, 21:].all() and d[1].sum() == 255 * 15
    assert np.array_equal(ref.dilate(m, 0), m)
    assert np.array_equal(ref.finish(m, 2, True), 255 - d)
    brute = np.zeros_like(m)
    for y in range(16):
        for x in range(24):
            brute[:, y, x] = m[:, max(0, y - 3):y + 4, max(0, x - 3):x + 4].max(axis=(1, 2))
    assert np.array_equal(ref.dilate(m, 3), brute)


# ---- 2. host logic -----------------------------------------------------------------------------------
def test_constants_agree_with_the_restatement():
    from ccedit_amd import masktrack
    for name in ("CANDIDATES", "BOX", "FB_LIMIT", "VEC_MAX", "DILATE_MAX"):
        assert getattr(masktrack, name) == getattr(ref, name), name
    src = open(os.path.join(ROOT, "ccedit_amd", "csrc", "masktrack.hip")).read()
    assert re.search(r"kVecMax = %d;" % ref.VEC_MAX, src)
    ys, xs = [c[0] for c in ref.CANDIDATES], [c[1] for c in ref.CANDIDATES]
    assert "kOrderY = pack9(%s)" % ", ".join(map(str, ys)) in src and "kOrderX = pack9(%s)" % ", ".join(map(str, xs)) in src


def test_chain_and_pair_rows():
    from ccedit_amd.masktrack import chain, pair_rows
    assert chain(5, 0) == [(1, 0), (2, 1), (3, 2), (4, 3)]
    assert chain(5, 4) == [(3, 4), (2, 3), (1, 2), (0, 1)]
    assert chain(5, 2) == [(3, 2), (4, 3), (1, 2), (0, 1)]
    assert chain(1, 0) == [] and pair_rows(1, 0).shape == (0, 4)
    for frames, anchor in ((5, 2), (7, 0), (113, 56)):
        rows = pair_rows(frames, anchor)
        assert rows.dtype == np.int32 and rows.shape == (2 * (frames - 1), 4)
        assert np.array_equal(rows[0::2, :2], rows[1::2, 1::-1]), "row 2 i + 1 is the way back of row 2 i"
        assert sorted(map(tuple, rows[:, :2])) == sorted([(f, f - 1) for f in range(1, frames)] + [(f - 1, f) for f in range(1, frames)])
        known = {anchor}
        for f, g in rows[0::2, :2]:
            assert g in known and f not in known, "a frame is tracked from a neighbour whose mask exists"
            known.add(int(f))
        assert known == set(range(frames))
    for frames, anchor in ((5, 5), (5, -1), (0, 0)):
        with pytest.raises(ValueError):
            chain(frames, anchor)
    with pytest.raises(ValueError, match="--mask_frame 9 is outside the video's 5 frames"):
        pair_rows(5, 9)


def test_size_and_dilate_refusals():
    from ccedit_amd import masktrack
    masktrack.check_size(64, 128)
    for h, w in ((64, 96), (0, 64), (72, 64)):
        with pytest.raises(ValueError, match="multiples of 64"):
            masktrack.check_size(h, w)
    for r in (0, 32):
        masktrack.check_dilate(r)
    for r in (-1, 33):
        with pytest.raises(ValueError, match="--mask_dilate"):
            masktrack.check_dilate(r)
    m = object()
    assert masktrack.finish(m, 0, False) is m, "the defaults are the identity"


# ---- 3. the command line -----------------------------------------------------------------------------
def test_both_entry_points_accept_the_flags_and_refuse_bad_combinations():
    from scripts.sampling import sampling_tv2v as S
    from scripts.sampling import sampling_tv2v_ref as R
    for mod in (S, R):
        a = mod.parse_args([])
        assert (a.mask_track, a.mask_frame, a.mask_dilate, a.mask_invert) == (False, 0, 0, False)
        a = mod.parse_args(["--inpainting_mode", "--mask_track", "--mask_frame", "5", "--mask_dilate", "3", "--mask_invert"])
        assert (a.mask_track, a.mask_frame, a.mask_dilate, a.mask_invert) == (True, 5, 3, True)
        with pytest.raises(ValueError, match="--inpainting_mode"):
            mod.parse_args(["--mask_track"])
        with pytest.raises(ValueError, match="multiples of 64"):
            mod.parse_args(["--inpainting_mode", "--mask_track", "--H", "200"])
        with pytest.raises(ValueError, match="--mask_dilate"):
            mod.parse_args(["--mask_dilate", "40"])
        with pytest.raises(ValueError, match="--mask_frame"):
            mod.parse_args(["--inpainting_mode", "--mask_track", "--mask_frame", "-1"])


def test_a_mask_sequence_is_refused_before_the_video_is_read(tmp_path):
    import argparse
    import torch
    from PIL import Image
    from scripts.sampling import sampling_tv2v as S
    d = tmp_path / "masks"
    d.mkdir()
    for i in range(3):
        Image.fromarray(np.zeros((64, 64), np.uint8)).save(str(d / f"{i:03d}.png"))
    args = argparse.Namespace(H=64, W=64, original_fps=20, target_fps=10, num_keyframes=3, inpainting_mode=True, mask_path=str(d), mask_root="",
                              gpu_io=False, mask_track=True, mask_frame=0, mask_dilate=0, mask_invert=False)
    with pytest.raises(ValueError, match="one image"):
        S.clip_masks(args, [str(tmp_path / "no_such_clip.gif")], torch.device("cpu"))


# ---- 4. the C ABI ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from ccedit_amd.csrc.build import build
    build(force=False, verbose=False)
    from ccedit_amd import hip
    return hip.lib()


def test_symbols_declared_exported_bound_and_built_like_propagate(lib):
    from ccedit_amd import hip, ops
    from ccedit_amd.csrc import build
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ccedit_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(hip.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/ccedit_hip.h"
        assert hasattr(raw, name), f"{name} is not exported by the library"
        assert name in hip.EXPORTS
    for name in ("masktrack_select", "masktrack_step", "mask_dilate"):
        assert callable(getattr(ops, name))
    assert "masktrack.hip" in build.SOURCES and build.EXTRA_FLAGS["masktrack.hip"] == build.EXTRA_FLAGS["propagate.hip"]
    assert lib.ccedit_abi_version() == 12


def test_arguments_are_validated_before_any_hip_call(lib):
    P = 64          # any non-null, 16-byte aligned "pointer": nothing is dereferenced before the checks fail

    def err():
        return lib.ccedit_last_error()
    assert lib.ccedit_masktrack_select(None, P, P, P, 2, 3, 64, 64, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_masktrack_select(P, P, P, P, 0, 3, 64, 64, None) == -1 and b"pairs" in err()
    assert lib.ccedit_masktrack_select(P, P, P, P, 2, 3, 64, 96, None) == -1 and b"multiples of 64" in err()
    assert lib.ccedit_masktrack_select(P, P, P, P + 2, 2, 3, 64, 64, None) == -1 and b"aligned" in err()
    assert lib.ccedit_masktrack_step(P, P, None, P * 2, 64, 64, 1, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_masktrack_step(P, P, P, P * 2, 64, 72, 1, None) == -1 and b"multiples of 64" in err()
    assert lib.ccedit_masktrack_step(P, P, P, P * 2, 64, 64, -1, None) == -1 and b"limit" in err()
    assert lib.ccedit_masktrack_step(P + 4, P, P, P * 2, 64, 64, 1, None) == -1 and b"aligned" in err()
    assert lib.ccedit_masktrack_step(P, P, P, P, 64, 64, 1, None) == -1 and b"two buffers" in err()
    assert lib.ccedit_mask_dilate(None, P, P * 2, 1, 64, 64, 1, 0, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_mask_dilate(P, None, P * 2, 1, 64, 64, 1, 0, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_mask_dilate(P, P * 3, P * 2, 1, 64, 62, 1, 0, None) == -1 and b"multiple of 4" in err()
    assert lib.ccedit_mask_dilate(P, P * 3, P * 2, 1, 64, 64, 33, 0, None) == -1 and b"0 ... 32" in err()
    assert lib.ccedit_mask_dilate(P, P * 3, P * 2, 1, 64, 64, 1, 2, None) == -1 and b"invert" in err()
    assert lib.ccedit_mask_dilate(P, P * 3, P, 1, 64, 64, 1, 0, None) == -1 and b"different buffers" in err()
