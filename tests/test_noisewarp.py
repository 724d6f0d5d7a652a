"""Motion-following noise (`--noise_warp`), the parts that can be checked without a GPU: the properties of the numpy restatement
(tests/_noisewarp_numpy.py) that make it worth matching — every frame reads distinct samples, a still clip inherits everything, noise
inherits nothing, and on a moving scene most cells inherit —, the host logic of ccedit_amd/noisewarp.py (constants, refusals), the
command-line surface of both entry points, and the five C-ABI entry points: declared, exported, bound, arguments validated before
any HIP call.

The bound on the inherited share (0.75 per keyframe after the first, on scene(128, 192, 13, seed=3) with every third frame a
keyframe) is the issue's; the restatement gives 0.932, 0.859, 0.935, 0.833 (printed by the test)."""
import argparse
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _noisewarp_numpy as ref  # noqa: E402
from _masktrack_scenes import random_frames, scene  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ("ccedit_noisewarp_track", "ccedit_noisewarp_claim", "ccedit_noisewarp_resolve", "ccedit_noisewarp_check", "ccedit_noise_warp")
KEYS = (0, 3, 6, 9, 12)
CELLS = (128 // 8) * (192 // 8)


@functools.lru_cache(maxsize=None)
def _built(kind):
    """(src, shares) of the restatement on a clip of 13 frames of 128 x 192 — computed once, shared and never written to."""
    if kind == "scene":
        frames = scene(128, 192, 13, seed=3)[0]
    elif kind == "still":
        frames = np.repeat(scene(128, 192, 1, seed=3)[0], 13, axis=0)
    else:
        frames = random_frames(128, 192, 13, 5)
    return ref.build(frames, KEYS)


# ---- 1. properties of the restatement ----------------------------------------------------------------
def test_constants_are_the_modules():
    from ccedit_amd import noisewarp
    for name in ("CELL", "FB_LIMIT", "VEC_MAX", "TABLE_MAX"):
        assert getattr(noisewarp, name) == getattr(ref, name), name
    assert (ref.CELL, ref.FB_LIMIT, ref.VEC_MAX, ref.TABLE_MAX) == (8, 4, 64, 2 ** 32 - 1)
    from ccedit_amd.masktrack import pair_rows
    assert [tuple(r[:2]) for r in pair_rows(5, 0)] == ref.pair_rows(5), "the row order is masktrack.pair_rows' with the anchor at frame 0"


def test_a_moving_scene_inherits_most_cells_and_every_frame_reads_distinct_samples():
    src, shares = _built("scene")
    print("inherited share per keyframe:", [round(float(s), 3) for s in shares])
    assert src.shape == (5, CELLS) and src.dtype == np.int32
    for k in range(5):
        assert len(np.unique(src[k])) == CELLS, f"keyframe {k} reads a sample twice"
        assert src[k].min() >= 0 and src[k].max() < (k + 1) * CELLS, "a sample comes from this keyframe or an earlier one"
    assert shares[0] == 0.0 and np.array_equal(src[0], np.arange(CELLS))
    assert min(shares[1:]) >= 0.75, shares
    fresh = src >= (np.arange(5) * CELLS)[:, None]
    assert np.array_equal(src[fresh], (np.arange(5)[:, None] * CELLS + np.arange(CELLS))[fresh]), "a fresh cell reads its own sample"
    assert np.allclose(shares, 1.0 - fresh.mean(axis=1))


def test_a_still_clip_inherits_everything_and_noise_inherits_nothing():
    src, shares = _built("still")
    assert all(np.array_equal(s, np.arange(CELLS)) for s in src) and list(shares) == [0.0, 1.0, 1.0, 1.0, 1.0]
    src, shares = _built("random")
    assert np.array_equal(src.reshape(-1), np.arange(5 * CELLS)) and not np.any(shares), "unmatched content: the map is the identity"


def test_many_cells_arriving_at_one_sample_the_smallest_index_keeps_it():
    h = w = 64
    trk = np.zeros((2, 64, 3), np.int32)
    trk[1] = (1, 8 * 3 + 4, 8 * 5 + 4)                               # every cell arrives at the centre of cell (3, 5)
    org, src, inherited = ref.origins(trk, h, w)
    assert inherited.tolist() == [0, 1] and src[1, 0] == 3 * 8 + 5 and org[1, 0].tolist() == [0, 28, 44]
    assert np.array_equal(src[1, 1:], 64 + np.arange(1, 64)) and len(np.unique(src[1])) == 64
    trk[1, :, 1:] += 3                                               # off centre by (3, 3): the sample's position moves with it
    assert ref.origins(trk, h, w)[0][1, 0].tolist() == [0, 31, 47]
    trk[1, :, 0] = 0                                                 # no valid track: everything is fresh
    assert np.array_equal(ref.origins(trk, h, w)[1].reshape(-1), np.arange(128))


def test_track_forward_backward_limit_and_the_frame_border():
    h, w = 64, 128
    vec = np.zeros((2, 8, 16, 2), np.int32)
    t = ref.track(vec, [0, 1], h, w)
    cy, cx = ref.centres(8, 16)
    assert t[1, :, 0].all() and np.array_equal(t[1, :, 1], cy) and np.array_equal(t[1, :, 2], cx) and not t[0].any()
    vec[0], vec[1] = (8, -16), (-8, 16)
    t = ref.track(vec, [0, 1], h, w)
    inside = (cy + 8 < h) & (cx - 16 >= 0)
    assert np.array_equal(t[1, :, 0] != 0, inside) and 0 < inside.sum() < inside.size
    vec[0], vec[1] = (200, -200), (-200, 200)
    clamped = vec.copy()
    clamped[0], clamped[1] = (64, -64), (-64, 64)
    assert np.array_equal(ref.track(vec, [0, 1], h, w), ref.track(clamped, [0, 1], h, w))
    vec[0], vec[1] = (0, 0), (3, -2)
    assert not ref.track(vec, [0, 1], h, w)[1, :, 0].any(), "|v + r| = 5 is dropped"
    vec[1] = (3, -1)
    assert ref.track(vec, [0, 1], h, w)[1, :, 0].all(), "|v + r| = 4 is kept"


def test_gather_is_a_bit_copy():
    rs = np.random.RandomState(1)
    raw = rs.randint(-2 ** 31, 2 ** 31, (2, 3, 2, 2, 4), dtype=np.int64).astype(np.int32).view(np.float32)
    src = np.stack([rs.permutation(16), np.arange(16)[::-1]]).astype(np.int32).reshape(2, 2, 8)
    out = ref.gather(raw, src)
    assert out.dtype == np.float32 and out.shape == raw.shape
    flat_in, flat_out = raw.view(np.int32).reshape(2, 3, 16), out.view(np.int32).reshape(2, 3, 16)
    for b in range(2):
        assert np.array_equal(flat_out[b], flat_in[b][:, src[b].reshape(-1)])


# ---- 2. the host logic ---------------------------------------------------------------------------------
def test_refusals_of_the_module():
    from ccedit_amd import noisewarp
    for rho in (0.0, 0.5, 1.0, 1):
        noisewarp.check_rho(rho)
    for rho in (-0.01, 1.01, float("nan"), None):
        with pytest.raises(ValueError, match="--noise_warp_rho"):
            noisewarp.check_rho(rho)
    noisewarp.check_clip(17, 512, 768)
    with pytest.raises(ValueError, match="multiples of 64"):
        noisewarp.check_clip(5, 96, 128)
    with pytest.raises(ValueError, match="32-bit"):
        noisewarp.check_clip(65535, 8192, 8192)
    assert noisewarp.keys_of([0, 3, 6], 7).tolist() == [0, 3, 6]
    with pytest.raises(ValueError, match="strictly increasing"):
        noisewarp.keys_of([0, 2, 2], 7)
    with pytest.raises(ValueError, match="outside"):
        noisewarp.keys_of([0, 7], 7)


# ---- 3. the command line -----------------------------------------------------------------------------
VIDEO = ["--video_path", "clip.gif", "--H", "128", "--W", "192"]


def test_both_entry_points_accept_the_flags_and_refuse_bad_combinations(monkeypatch):
    from scripts.sampling import sampling_tv2v as S
    from scripts.sampling import sampling_tv2v_ref as R
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for mod in (S, R):
        a = mod.parse_args([])
        assert (a.noise_warp, a.noise_warp_rho) == (False, 1.0)
        a = mod.parse_args(["--noise_warp"] + VIDEO)
        assert (a.noise_warp, a.noise_warp_rho) == (True, 1.0)
        a = mod.parse_args(["--noise_warp", "--noise_warp_rho", "0.25"] + VIDEO)
        assert (a.noise_warp, a.noise_warp_rho) == (True, 0.25)
        with pytest.raises(ValueError, match="give --noise_warp too"):
            mod.parse_args(["--noise_warp_rho", "1.0"] + VIDEO)
        with pytest.raises(ValueError, match="give --video_path"):
            mod.parse_args(["--noise_warp", "--H", "128", "--W", "192"])
        for size in (["--H", "96", "--W", "192"], ["--H", "128", "--W", "200"]):
            with pytest.raises(ValueError, match="multiples of 64"):
                mod.parse_args(["--noise_warp", "--video_path", "clip.gif"] + size)
        for rho in ("-0.5", "1.5"):
            with pytest.raises(ValueError, match="outside 0 ... 1"):
                mod.parse_args(["--noise_warp", f"--noise_warp_rho={rho}"] + VIDEO)
    args = S.parse_args(["--noise_warp"] + VIDEO)
    S.check_noise_warp(args)
    with pytest.raises(ValueError, match="reference image"):
        S.check_noise_warp(args, with_ref=True)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="WORLD_SIZE"):
        S.check_noise_warp(args)
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(ValueError, match="give --video_path"):
        S.noise_map(argparse.Namespace(**dict(vars(args), video_path="")), "", None)


def test_the_reference_image_script_refuses_the_flag_before_any_gpu_work(monkeypatch):
    from scripts.sampling import sampling_tv2v_ref as R
    monkeypatch.setattr(sys, "argv", ["sampling_tv2v_ref.py", "--noise_warp", "--synthetic"] + VIDEO)
    monkeypatch.setattr(R, "build_model", lambda *a, **k: pytest.fail("the model was built"))
    with pytest.raises(ValueError, match="reference image"):
        R.main()


def test_without_the_flag_the_module_is_not_imported():
    code = ("import sys; sys.path.insert(0, %r); from scripts.sampling import sampling_tv2v as S; "
            "a = S.parse_args(['--synthetic', '--video_path', 'clip.gif', '--prompt', 'x', '--H', '128', '--W', '192']); S.check_noise_warp(a); "
            "assert not S.noise_warp_on(a); print('ccedit_amd.noisewarp' in sys.modules); "
            "S.parse_args(['--noise_warp', '--video_path', 'clip.gif', '--H', '128', '--W', '192']); print('ccedit_amd.noisewarp' in sys.modules)" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["False", "True"]


def test_sdedit_start_takes_a_noise_source_and_defaults_to_none():
    import inspect
    from scripts.sampling.util import sdedit_start
    p = inspect.signature(sdedit_start).parameters
    assert list(p) == ["model", "sampler", "keyframes", "noise"] and p["noise"].default is None


# ---- 4. the C ABI ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from ccedit_amd.csrc.build import build
    build(force=False, verbose=False)
    from ccedit_amd import hip
    return hip.lib()


def test_symbols_declared_exported_bound_and_built_like_masktrack(lib):
    from ccedit_amd import hip, ops
    from ccedit_amd.csrc import build
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ccedit_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(hip.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/ccedit_hip.h"
        assert hasattr(raw, name), f"{name} is not exported by the library"
        assert name in hip.EXPORTS
    for name in ("noisewarp_track", "noisewarp_origins", "noisewarp_check", "noise_warp"):
        assert callable(getattr(ops, name))
    assert "noisewarp.hip" in build.SOURCES and build.EXTRA_FLAGS["noisewarp.hip"] == build.EXTRA_FLAGS["masktrack.hip"]
    assert lib.ccedit_abi_version() == 12


def test_arguments_are_validated_before_any_hip_call(lib):
    P = 64          # any non-null, 16-byte aligned "pointer": nothing is dereferenced before the checks fail

    def err():
        return lib.ccedit_last_error()
    assert lib.ccedit_noisewarp_track(None, P, P, 3, 7, 64, 64, 4, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_noisewarp_track(P, P, P, 1, 7, 64, 64, 4, None) == -1 and b"keyframes" in err()
    assert lib.ccedit_noisewarp_track(P, P, P, 8, 7, 64, 64, 4, None) == -1 and b"K <= F" in err()
    assert lib.ccedit_noisewarp_track(P, P, P, 3, 7, 64, 96, 4, None) == -1 and b"multiples of 64" in err()
    assert lib.ccedit_noisewarp_track(P, P, P, 3, 7, 64, 64, -1, None) == -1 and b"limit" in err()
    assert lib.ccedit_noisewarp_track(P, P, P, 65535, 65535, 8192, 8192, 4, None) == -1 and b"int32" in err()
    assert lib.ccedit_noisewarp_claim(P, None, P, 1, 3, 64, 64, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_noisewarp_claim(P, P, P, 0, 3, 64, 64, None) == -1 and b"keyframe 0 inherits nothing" in err()
    assert lib.ccedit_noisewarp_claim(P, P, P, 3, 3, 64, 64, None) == -1 and b"k=3" in err()
    assert lib.ccedit_noisewarp_claim(P, P, P + 2, 1, 3, 64, 64, None) == -1 and b"aligned" in err()
    assert lib.ccedit_noisewarp_resolve(P, P, P, P, None, 0, 3, 64, 64, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_noisewarp_resolve(P, P, P, P, P, -1, 3, 64, 64, None) == -1 and b"k=-1" in err()
    assert lib.ccedit_noisewarp_resolve(P, P, P, P, P, 0, 3, 72, 64, None) == -1 and b"multiples of 64" in err()
    assert lib.ccedit_noisewarp_check(None, 1, 64, P, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_noisewarp_check(P, 1, 2 ** 31, P, None) == -1 and b"below 2^31" in err()
    assert lib.ccedit_noise_warp(P, P, None, 1, 4, 64, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_noise_warp(P, P, P * 2, 0, 4, 64, None) == -1 and b"positive" in err()
    assert lib.ccedit_noise_warp(P, P, P * 2, 1, 4, 2 ** 31, None) == -1 and b"int32" in err()
    assert lib.ccedit_noise_warp(P, P + 2, P * 2, 1, 4, 64, None) == -1 and b"aligned" in err()
    assert lib.ccedit_noise_warp(P, P, P, 1, 4, 64, None) == -1 and b"two buffers" in err()
