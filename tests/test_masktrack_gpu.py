"""Mask tracking on a real MI355X (ccedit_amd/masktrack.py, csrc/masktrack.hip, ccedit_mask_dilate, --mask_track).

Exact (no tolerance anywhere): every entry point and track_clip as a whole against the numpy restatement (tests/_masktrack_numpy.py,
whose own properties tests/test_masktrack.py checks) on random bytes and on scenes — an object moving over a moving background — at
64 x 64, 64 x 128 and 128 x 192.  Also: block vectors that point outside the frame and garbage vectors are clamped and not followed,
the forward-backward limit sits exactly between |v + r| = 1 and 2, the result does not depend on the pair chunking, and clip_masks
of the entry point on a small gif."""
import argparse
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _masktrack_numpy as ref  # noqa: E402
from _masktrack_scenes import random_frames, scene  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(64, 64), (64, 128), (128, 192)]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _clip(kind, h, w, frames):
    """(frames, truth masks, pyramids) — computed once, shared and never written to."""
    if kind == "random":
        src, truth = random_frames(h, w, frames, 11), None
    else:
        src, truth = scene(h, w, frames, 3, bg=(1, -2), obj=(-2, 3))
    return src, truth, [ref.pyramid(ref.luma(f)) for f in src]


@functools.lru_cache(maxsize=None)
def _tracked(h, w, frames, anchor):
    src, truth, _ = _clip("scene", h, w, frames)
    return ref.track(src, truth[anchor], anchor)


# ---- 1. select ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("kind", ["random", "scene"])
@pytest.mark.parametrize("vectors", ["matched", "outside", "garbage"])
def test_select_is_exact(h, w, kind, vectors):
    """Pairs (1 -> 0), (0 -> 1), (2 -> 1).  Block vectors: the matcher's own; random ones up to +-64 (beyond the frame at 64 x 64, and
    the clamp's edge); any int32 (clamped into +-64 by the kernel as by the restatement, never followed)."""
    _need_gpu()
    from ccedit_amd import ops
    src, _, pyr_np = _clip(kind, h, w, 3)
    rows = np.asarray([(1, 0, 0, 0), (0, 1, 0, 0), (2, 1, 0, 0)], np.int32)
    rs = np.random.RandomState(5)
    if vectors == "matched":
        vec = np.stack([ref.match(pyr_np[f], pyr_np[k]) for f, k, _, _ in rows]).astype(np.int32)
    elif vectors == "outside":
        vec = rs.randint(-64, 65, (3, h // 8, w // 8, 2)).astype(np.int32)
        vec[0, 0, 0] = (-64, -64)
        vec[0, -1, -1] = (64, 64)
    else:
        vec = rs.randint(-2 ** 31, 2 ** 31, (3, h // 8, w // 8, 2), dtype=np.int64).astype(np.int32)
        vec[1, 0, 0] = (2 ** 31 - 1, -2 ** 31)
    pyr = ops.prop_pyramid(_dev(src))
    got = ops.masktrack_select(pyr, _dev(rows), _dev(vec), 3, h, w).cpu().numpy()
    assert got.dtype == np.int16 and got.shape == (3, h, w, 2)
    for i, (f, k, _, _) in enumerate(rows):
        want = ref.select(pyr_np[f][0], pyr_np[k][0], vec[i])
        assert np.array_equal(got[i], want), (kind, vectors, h, w, i, int((got[i] != want).any(axis=-1).sum()))
    if vectors == "matched" and kind == "scene":
        assert np.abs(got).max() > 0, "the scene moves: some vector must be non-zero"
        assert len({tuple(v) for v in got[0].reshape(-1, 2)}) > 1, "object and background move differently"


def test_select_follows_the_pair_list_and_clamps_it():
    """Frame numbers outside the pyramid are clamped into it, not followed."""
    _need_gpu()
    from ccedit_amd import ops
    h, w = 64, 128
    src, _, pyr_np = _clip("scene", h, w, 3)
    rows = np.asarray([(2, 0, 7, 7), (-5, 99, 0, 0)], np.int32)                     # the second: (0, 2) after clamping
    vec = np.random.RandomState(2).randint(-6, 7, (2, h // 8, w // 8, 2)).astype(np.int32)
    got = ops.masktrack_select(ops.prop_pyramid(_dev(src)), _dev(rows), _dev(vec), 3, h, w).cpu().numpy()
    assert np.array_equal(got[0], ref.select(pyr_np[2][0], pyr_np[0][0], vec[0]))
    assert np.array_equal(got[1], ref.select(pyr_np[0][0], pyr_np[2][0], vec[1]))


# ---- 2. step -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SIZES)
def test_step_forward_backward_limit_is_exact(h, w):
    """v is one vector everywhere, r = -v + e with |e|_1 drawn from 0 ... 3 per pixel: |v + r|_1 is exactly 1 (kept) and exactly 2
    (zeroed) on many pixels; then fields of any int16 (q is clamped into the frame)."""
    _need_gpu()
    from ccedit_amd import ops
    from ccedit_amd.masktrack import FB_LIMIT
    rs = np.random.RandomState(8)
    m_g = np.where(rs.rand(h, w) < 0.6, 255, 0).astype(np.uint8)
    errs = np.asarray([(0, 0), (1, 0), (0, -1), (-1, 0), (0, 1), (1, 1), (-1, 1), (2, 0), (0, -2), (2, -1), (-1, -2), (3, 0)], np.int16)
    e = errs[rs.randint(0, len(errs), (h, w))]
    v = np.broadcast_to(np.asarray((2, -3), np.int16), (h, w, 2)).copy()
    r = (-v + e).astype(np.int16)
    got = ops.masktrack_step(_dev(v), _dev(r), _dev(m_g), FB_LIMIT).cpu().numpy()
    want = ref.step(m_g, v, r)
    assert np.array_equal(got, want)
    qy, qx = np.clip(np.arange(h)[:, None] + 2, 0, h - 1), np.clip(np.arange(w)[None, :] - 3, 0, w - 1)
    n1 = np.abs(e[qy, qx]).sum(-1)
    assert (n1 == 1).any() and (n1 == 2).any()
    assert np.array_equal(got[n1 == 1], m_g[qy, qx][n1 == 1]), "|v + r| = 1 is kept"
    assert not got[n1 == 2].any() and m_g[qy, qx][n1 == 2].any(), "|v + r| = 2 is cleared"
    for seed in (1, 2):
        rs = np.random.RandomState(seed)
        v = rs.randint(-2 ** 15, 2 ** 15, (h, w, 2)).astype(np.int16) if seed == 1 else rs.randint(-70, 71, (h, w, 2)).astype(np.int16)
        r = rs.randint(-70, 71, (h, w, 2)).astype(np.int16)
        for limit in (FB_LIMIT, 40, 10 ** 9):
            got = ops.masktrack_step(_dev(v), _dev(r), _dev(m_g), limit).cpu().numpy()
            assert np.array_equal(got, ref.step(m_g, v, r, limit)), (seed, limit)


# ---- 3. track_clip -----------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,frames,anchor", [(64, 64, 7, 0), (64, 128, 7, 3), (64, 128, 7, 6), (128, 192, 13, 6)])
def test_track_clip_is_exact_and_independent_of_the_chunking(h, w, frames, anchor):
    _need_gpu()
    from ccedit_amd.masktrack import track_clip
    src, truth, _ = _clip("scene", h, w, frames)
    want = _tracked(h, w, frames, anchor)
    dsrc, dmask = _dev(src), _dev(truth[anchor])
    for chunk in (2, 6, None):
        got = track_clip(dsrc, dmask, anchor, pair_chunk=chunk).cpu().numpy()
        assert got.shape == (frames, h, w)
        assert np.array_equal(got[anchor], truth[anchor])
        assert np.array_equal(got, want), (chunk, [int((got[f] != want[f]).sum()) for f in range(frames)])
    assert set(np.unique(want)) <= {0, 255}                                        # (how well it tracks: tests/test_masktrack.py)


def test_track_clip_single_frame_and_refusals():
    _need_gpu()
    from ccedit_amd.masktrack import track_clip
    src, truth, _ = _clip("scene", 64, 64, 7)
    one = track_clip(_dev(src[:1]), _dev(truth[0]), 0).cpu().numpy()
    assert np.array_equal(one[0], truth[0])
    with pytest.raises(ValueError, match="--mask_frame"):
        track_clip(_dev(src), _dev(truth[0]), 7)
    with pytest.raises(ValueError, match="pair_chunk"):
        track_clip(_dev(src), _dev(truth[0]), 0, pair_chunk=3)
    with pytest.raises(ValueError, match="multiples of 64"):
        track_clip(_dev(src[:, :56]), _dev(truth[0][:56]), 0)
    with pytest.raises(ValueError, match="anchor_mask"):
        track_clip(_dev(src), _dev(truth[0][:32]), 0)


# ---- 4. dilate, invert -------------------------------------------------------------------------------
def _corner_masks(h, w):
    m = np.zeros((3, h, w), np.uint8)
    m[0, 0, 0] = m[0, 0, w - 1] = m[0, h - 1, 0] = m[0, h - 1, w - 1] = 255          # the corners
    m[1, 0, w // 2] = m[1, h - 1, 5] = m[1, h // 3, 0] = m[1, 7, w - 1] = 255        # the edges
    m[2] = np.where(np.random.RandomState(4).rand(h, w) < 0.002, 255, 0)
    m[2, h // 2, w // 2] = 200                                                      # (a maximum of bytes, not of bits)
    return m


@pytest.mark.parametrize("radius", [0, 1, 3, 32])
@pytest.mark.parametrize("h,w", [(64, 64), (64, 128)])
def test_dilate_and_invert_are_exact(h, w, radius):
    _need_gpu()
    from ccedit_amd import ops
    m = _corner_masks(h, w)
    d = _dev(m)
    got = ops.mask_dilate(d, radius)
    if radius == 0:
        assert got is d, "radius 0 is the identity and launches nothing"
    assert np.array_equal(got.cpu().numpy(), ref.dilate(m, radius))
    assert np.array_equal(ops.mask_dilate(d, radius, invert=True).cpu().numpy(), ref.finish(m, radius, True))
    assert np.array_equal(d.cpu().numpy(), m), "the input is left alone"
    four = m.reshape(1, 3, h, w)
    assert np.array_equal(ops.mask_dilate(_dev(four), radius, invert=True).cpu().numpy(), ref.finish(four, radius, True))


def test_dilate_refuses_bad_arguments():
    _need_gpu()
    from ccedit_amd import ops
    d = _dev(_corner_masks(64, 64))
    for radius in (-1, 33):
        with pytest.raises(ValueError, match="0 ... 32"):
            ops.mask_dilate(d, radius)


# ---- 5. the entry point's clip_masks -----------------------------------------------------------------
def _args(**kw):
    base = dict(H=64, W=64, original_fps=20, target_fps=10, num_keyframes=3, inpainting_mode=True, mask_path="", mask_root="", gpu_io=False,
                mask_track=False, mask_frame=0, mask_dilate=0, mask_invert=False, gif_decoder="pillow")
    base.update(kw)
    return argparse.Namespace(**base)


@pytest.fixture(scope="module")
def gif_clip(tmp_path_factory):
    from PIL import Image
    d = tmp_path_factory.mktemp("masktrack")
    src, truth, _ = _clip("scene", 64, 64, 7)
    video, mask = str(d / "clip.gif"), str(d / "painted.png")
    frames = [Image.fromarray(f) for f in src]
    frames[0].save(video, save_all=True, append_images=frames[1:], duration=50, loop=0)
    Image.fromarray(truth[3]).save(mask)
    return video, mask, truth


def test_clip_masks_tracks_the_painted_frame(gif_clip):
    """No network evaluation: clip_masks alone, keyframes 0, 2, 4 of 7, the mask painted on frame 3."""
    _need_gpu()
    from scripts.sampling import sampling_tv2v as S
    from scripts.sampling.util import load_video_frames_u8
    video, mask, truth = gif_clip
    dev = torch.device("cuda", torch.cuda.current_device())
    frames = load_video_frames_u8(video, (64, 64), dev).cpu().numpy()
    want = ref.track(frames, truth[3], 3)
    got = S.clip_masks(_args(mask_path=mask, mask_track=True, mask_frame=3), [video], dev)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (1, 3, 64, 64)
    assert np.array_equal(got[0].cpu().numpy(), want[[0, 2, 4]])
    assert ref.iou(want[0], truth[0]) > ref.iou(truth[3], truth[0]), "the tracked mask follows the object, the painted one held still does not"
    full = S.all_frame_masks(_args(mask_path=mask, mask_track=True, mask_frame=3, mask_composite=True), video, 7, dev)
    assert np.array_equal(full.cpu().numpy(), want)
    post = S.clip_masks(_args(mask_path=mask, mask_track=True, mask_frame=3, mask_dilate=2, mask_invert=True), [video], dev)
    assert np.array_equal(post[0].cpu().numpy(), ref.finish(want[[0, 2, 4]], 2, True))


def test_clip_masks_without_the_flag_repeats_the_image(gif_clip):
    _need_gpu()
    from scripts.sampling import sampling_tv2v as S
    video, mask, truth = gif_clip
    dev = torch.device("cuda", torch.cuda.current_device())
    for extra in ({}, {"gpu_io": True}):
        got = S.clip_masks(_args(mask_path=mask, **extra), [video], dev)
        assert np.array_equal(got.cpu().numpy(), np.broadcast_to(truth[3], (1, 3, 64, 64)))
    grown = S.clip_masks(_args(mask_path=mask, mask_dilate=3), [video], dev)                 # the new flags apply to untracked masks too
    assert np.array_equal(grown.cpu().numpy(), np.broadcast_to(ref.dilate(truth[3], 3), (1, 3, 64, 64)))


def test_clip_masks_refusals(gif_clip, tmp_path):
    _need_gpu()
    from PIL import Image
    from scripts.sampling import sampling_tv2v as S
    video, mask, truth = gif_clip
    dev = torch.device("cuda", torch.cuda.current_device())
    seq = str(tmp_path / "masks.gif")
    ms = [Image.fromarray(m) for m in truth]
    ms[0].save(seq, save_all=True, append_images=ms[1:], duration=50, loop=0)
    with pytest.raises(ValueError, match="sequence"):
        S.clip_masks(_args(mask_path=seq, mask_track=True), [video], dev)
    with pytest.raises(ValueError, match="--mask_frame"):
        S.clip_masks(_args(mask_path=mask, mask_track=True, mask_frame=7), [video], dev)
    with pytest.raises(ValueError, match="--inpainting_mode"):
        S.clip_masks(_args(mask_path=mask, mask_track=True, inpainting_mode=False), [video], dev)
    with pytest.raises(ValueError, match="multiples of 64"):
        S.clip_masks(_args(mask_path=mask, mask_track=True, W=96), [video], dev)
    with pytest.raises(ValueError, match="--mask_dilate"):
        S.clip_masks(_args(mask_path=mask, mask_dilate=33), [video], dev)
