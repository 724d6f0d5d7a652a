"""Graded edit masks (`--mask_graded`, `--mask_feather`), the parts that can be checked without a GPU: the per-step
thresholds of ccedit_amd/softmask.py, the numpy restatement itself (tests/_softmask_numpy.py: feather, latent strengths) on cases
whose answer is known in closed form, the command-line surface and the refusals of both entry points, and the four C-ABI entry points —
declared, exported, bound, arguments validated before any HIP call."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _softmask_numpy as ref  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ("ccedit_mask_feather", "ccedit_mask_latent_graded", "ccedit_mask_composite_graded", "ccedit_inpaint_blend_level")
STEPS = (1, 2, 7, 30, 50, 255, 300)


@pytest.fixture(scope="module")
def lib():
    from ccedit_amd.csrc.build import build
    build(force=False, verbose=False)
    from ccedit_amd import hip
    return hip.lib()


# ---- 1. thresholds ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", STEPS)
def test_threshold_starts_at_255_never_rises_and_stays_in_1_to_255(n):
    from ccedit_amd import softmask
    thr = softmask.thresholds(n)
    assert thr == [softmask.threshold(j, n) for j in range(n)] == [ref.threshold(j, n) for j in range(n)]
    assert thr[0] == 255
    assert all(a >= b for a, b in zip(thr, thr[1:]))
    assert all(1 <= t <= 255 for t in thr)
    for bad in ((-1, n), (n, n), (0, 0)):
        with pytest.raises(ValueError, match="walked steps"):
            softmask.threshold(*bad)


@pytest.mark.parametrize("n", STEPS)
def test_threshold_is_the_integer_form_of_the_rule(n):
    """L >= thr(j, n)  <=>  L n >= 255 (n - j), for every strength L and every walked step j."""
    from ccedit_amd import softmask
    L = np.arange(256, dtype=np.int64)[:, None]
    j = np.arange(n, dtype=np.int64)[None, :]
    thr = np.array(softmask.thresholds(n), dtype=np.int64)[None, :]
    assert np.array_equal(L >= thr, L * n >= 255 * (n - j))
    free = L >= thr
    assert free[255].all() and not free[0].any()                          # strength 255 is free from the first step, strength 0 never
    assert (free[:, 1:] >= free[:, :-1]).all()                            # once free, free


def test_check_feather_accepts_0_to_64():
    from ccedit_amd import softmask
    assert softmask.FEATHER_MAX == 64
    assert [softmask.check_feather(r) for r in (0, 1, 64)] == [0, 1, 64]
    for bad in (-1, 65, 1000):
        with pytest.raises(ValueError, match=r"0 \.\.\. 64"):
            softmask.check_feather(bad)


# ---- 2. the numpy definitions on cases with a known answer --------------------------------------
def _feather_brute(m, r):
    h, w = m.shape
    out = np.zeros_like(m)
    for y in range(h):
        for x in range(w):
            win = m[max(y - r, 0): y + r + 1, max(x - r, 0): x + r + 1].astype(np.int64)
            out[y, x] = (2 * win.sum() + win.size) // (2 * win.size)
    return out


def test_feather_constant_maps_are_fixed_points():
    for v in (0, 1, 127, 128, 254, 255):
        m = np.full((2, 12, 20), v, np.uint8)
        for r in (0, 1, 3, 64):
            assert np.array_equal(ref.feather(m, r), m), (v, r)


def test_feather_of_a_single_white_pixel():
    h, w, py, px, r = 16, 24, 2, 21, 3
    m = np.zeros((h, w), np.uint8)
    m[py, px] = 255
    out = ref.feather(m, r)
    for y in range(h):
        for x in range(w):
            a = (min(y + r, h - 1) - max(y - r, 0) + 1) * (min(x + r, w - 1) - max(x - r, 0) + 1)
            want = (2 * 255 + a) // (2 * a) if abs(y - py) <= r and abs(x - px) <= r else 0
            assert out[y, x] == want, (y, x)
    assert out[8, 10] == 0 and out[py, px] == (2 * 255 + 36) // 72           # the window at (2, 21) is clipped to 6 x 6


def test_feather_of_a_step_edge_is_a_ramp():
    r, w = 4, 40
    m = np.zeros((12, w), np.uint8)
    m[:, 20:] = 255
    out = ref.feather(m, r)
    for x in range(r, w - r):                                                  # away from the side borders: k white columns of 2r + 1
        k = min(max(x + r - 19, 0), 2 * r + 1)
        assert (out[:, x] == (2 * 255 * k + (2 * r + 1)) // (2 * (2 * r + 1))).all(), x
    assert (np.diff(out[6].astype(int)) >= 0).all() and out[6, 0] == 0 and out[6, -1] == 255
    assert np.array_equal(out, _feather_brute(m, r))


def test_feather_radius_larger_than_the_frame_and_random_bytes():
    rs = np.random.RandomState(5)
    m = rs.randint(0, 256, (8, 12)).astype(np.uint8)
    big = ref.feather(m, 64)                                                   # every window is the whole frame
    assert (big == (2 * int(m.sum()) + m.size) // (2 * m.size)).all()
    for r in (1, 3, 5):
        assert np.array_equal(ref.feather(m, r), _feather_brute(m, r)), r
    two = np.stack([m, 255 - m])
    assert np.array_equal(ref.feather(two, 3)[1], _feather_brute(255 - m, 3))  # per map: nothing crosses frames


def test_latent_strength_of_a_cell_aligned_binary_mask_is_255_times_the_binary_rule():
    rs = np.random.RandomState(3)
    cells = (rs.rand(2, 3, 5, 9) > 0.5)
    m = (cells.repeat(8, axis=2).repeat(8, axis=3) * 255).astype(np.uint8)
    L = ref.latent_strength(m)
    assert L.shape == (2, 3, 5, 9) and set(np.unique(L)) <= {0, 255}
    k = (m >= 128).reshape(2, 3, 5, 8, 9, 8).sum(axis=(3, 5))                  # the binary route: a cell is 1 when k > 32
    assert np.array_equal(L, 255 * (k > 32).astype(np.uint8))
    # the rounding: a cell summing to 64 g + 31 gives g, 64 g + 32 gives g + 1
    cell = np.zeros((8, 8), np.uint8)
    cell.flat[:3] = (200, 200, 15)                                             # 415 = 64 * 6 + 31
    assert ref.latent_strength(cell)[0, 0] == 6
    cell.flat[2] = 16
    assert ref.latent_strength(cell)[0, 0] == 7
    assert ref.latent_strength(np.full((8, 8), 255, np.uint8))[0, 0] == 255


# ---- 3. command line ----------------------------------------------------------------------------
def _entry_points():
    from scripts.sampling import sampling_tv2v as S
    from scripts.sampling import sampling_tv2v_ref as R
    return S, R


def test_both_entry_points_accept_the_flags_and_defaults_change_nothing():
    for mod in _entry_points():
        a = mod.parse_args([])
        assert a.mask_graded is False and a.mask_feather == 0
        b = mod.parse_args(["--inpainting_mode"])
        c = mod.parse_args(["--inpainting_mode", "--mask_graded", "--mask_feather", "8"])
        assert c.mask_graded is True and c.mask_feather == 8
        vb, vc = dict(vars(b)), dict(vars(c))
        for k in ("mask_graded", "mask_feather"):
            vb.pop(k), vc.pop(k)
        assert vb == vc                                                        # no other field moves with the flags
        va = dict(vars(a))
        assert {k: v for k, v in va.items() if k not in ("mask_graded", "mask_feather", "inpainting_mode")} \
            == {k: v for k, v in vb.items() if k != "inpainting_mode"}
        for flags in (["--mask_graded"], ["--mask_feather", "4"]):             # without --inpainting_mode: argparse's own error exit
            with pytest.raises(SystemExit) as e:
                mod.parse_args(flags)
            assert e.value.code == 2
    S = _entry_points()[0]
    assert not S.graded_on(S.parse_args(["--inpainting_mode"]))
    assert S.graded_on(S.parse_args(["--inpainting_mode", "--mask_graded"])) and S.graded_on(S.parse_args(["--inpainting_mode", "--mask_feather", "1"]))


def test_refusals_say_what_to_do(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for mod in _entry_points():
        with pytest.raises(ValueError, match=r"--mask_feather R instead"):
            mod.parse_args(["--inpainting_mode", "--mask_graded", "--mask_track", "--H", "64", "--W", "64"])
        job = ["--prompt", "a fox", "--video_path", "clips/fox", "--save_type", "gif", "--inpainting_mode", "--propagate", "--mask_composite"]
        for flags in (["--mask_graded"], ["--mask_feather", "8"]):
            with pytest.raises(ValueError, match=r"would flicker.*drop --mask_composite"):
                mod.parse_args(job + flags)
        mod.parse_args(job[:-1] + ["--mask_feather", "8"])                     # (--propagate without the composite is fine)
        for r in ("65", "-1", "1000"):
            with pytest.raises(ValueError, match=r"0 \.\.\. 64 pixels"):
                mod.parse_args(["--inpainting_mode", f"--mask_feather={r}"])
        monkeypatch.setenv("WORLD_SIZE", "2")
        for flags in (["--mask_graded"], ["--mask_feather", "8"]):
            with pytest.raises(ValueError, match=r"WORLD_SIZE > 1.*one process"):
                mod.parse_args(["--inpainting_mode"] + flags)
        mod.parse_args(["--inpainting_mode"])                                  # (a binary run is not refused there)
        monkeypatch.delenv("WORLD_SIZE")
        mod.parse_args(["--inpainting_mode", "--mask_track", "--mask_feather", "8", "--H", "64", "--W", "64"])     # tracked, then feathered


def test_sample_inpainting_takes_exactly_one_of_mask_and_strength():
    import torch
    from ccedit_amd.sampling import DPMPP2SAncestralSampler, EulerEDMSampler
    disc = {"target": "ccedit_amd.sampling.LegacyDDPMDiscretization"}
    x = torch.zeros(1, 4, 1, 2, 2)
    for cls in (DPMPP2SAncestralSampler, EulerEDMSampler):
        s = cls(discretization_config=disc, num_steps=3, device="cpu")
        for kw in ({}, dict(mask=torch.ones(1, 1, 2, 2, dtype=torch.uint8), strength=torch.ones(1, 1, 2, 2, dtype=torch.uint8))):
            with pytest.raises(ValueError, match="exactly one of mask= .* and strength="):
                s.sample_inpainting(None, x, {}, x0=x, **kw)


def test_load_video_mask_graded_keeps_the_luminance_bytes(tmp_path):
    from PIL import Image
    from scripts.sampling.util import load_video_mask
    rs = np.random.RandomState(1)
    grey = rs.randint(0, 256, (24, 40)).astype(np.uint8)
    Image.fromarray(grey).save(str(tmp_path / "one.png"))
    got = load_video_mask(str(tmp_path / "one.png"), 9, 3, 3, (24, 40), graded=True).numpy()
    assert got.shape == (3, 24, 40) and all(np.array_equal(f, grey) for f in got)
    cut = load_video_mask(str(tmp_path / "one.png"), 9, 3, 3, (24, 40)).numpy()
    assert np.array_equal(cut[0], np.where(grey >= 128, 255, 0))               # without the keyword: the cut at 128, as before
    small = load_video_mask(str(tmp_path / "one.png"), 9, 3, 3, (12, 20), graded=True).numpy()
    assert np.array_equal(small[0], np.array(Image.fromarray(grey).resize((20, 12), Image.NEAREST)))


# ---- 4. C ABI -----------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound(lib):
    from ccedit_amd import hip, ops
    from ccedit_amd.csrc import build
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ccedit_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(hip.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/ccedit_hip.h"
        assert hasattr(raw, name), f"{name} is not exported by the library"
        assert name in hip.EXPORTS
    for name in ("mask_feather", "mask_latent_graded", "inpaint_blend_level", "mask_composite_graded"):
        assert callable(getattr(ops, name))
    assert "softmask.hip" in build.SOURCES and build.EXTRA_FLAGS["softmask.hip"] == build.EXTRA_FLAGS["mask.hip"]
    assert "-ffp-contract=off" in build.EXTRA_FLAGS["softmask.hip"]
    assert lib.ccedit_abi_version() == 12          # additive: the ABI version does not move


def test_entry_points_validate_before_any_hip_call(lib):
    """Null pointers and impossible sizes: negative code + message, no launch (there is no GPU here)."""
    P, Q, S = 64, 128, 192          # non-null, 64-byte aligned "pointers": nothing is dereferenced before the checks fail

    def err():
        return lib.ccedit_last_error()
    assert lib.ccedit_mask_feather(None, Q, S, 1, 8, 8, 1, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_mask_feather(P, None, S, 1, 8, 8, 1, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_mask_feather(P, Q, None, 1, 8, 8, 1, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_mask_feather(P, Q, S, 1, 8, 10, 1, None) == -1 and b"multiple of 4" in err()
    assert lib.ccedit_mask_feather(P, Q, S, 0, 8, 8, 1, None) == -1 and b"positive" in err()
    assert lib.ccedit_mask_feather(P, Q, S, 1, 8, 8, 65, None) == -1 and b"radius=65" in err()
    assert lib.ccedit_mask_feather(P, Q, S, 1, 8, 8, -1, None) == -1 and b"radius=-1" in err()
    assert lib.ccedit_mask_feather(P + 2, Q, S, 1, 8, 8, 1, None) == -1 and b"4-byte aligned" in err()
    assert lib.ccedit_mask_feather(P, Q, P, 1, 8, 8, 1, None) == -1 and b"different buffers" in err()
    assert lib.ccedit_mask_latent_graded(None, Q, 1, 8, 8, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_mask_latent_graded(P, None, 1, 8, 8, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_mask_latent_graded(P, Q, 1, 12, 8, None) == -1 and b"multiples of 8" in err()
    assert lib.ccedit_mask_latent_graded(P, Q, 1, 8, 20, None) == -1 and b"multiples of 8" in err()
    assert lib.ccedit_mask_latent_graded(P, Q, 0, 8, 8, None) == -1 and b"multiples of 8" in err()
    assert lib.ccedit_mask_latent_graded(P + 4, Q, 1, 8, 8, None) == -1 and b"8-byte aligned" in err()
    assert lib.ccedit_mask_composite_graded(None, P, P, P, 1, 64, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_mask_composite_graded(P, P, None, P, 1, 64, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_mask_composite_graded(P, P, P, None, 1, 64, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_mask_composite_graded(P, P, P, P, 0, 64, None) == -1 and b"B=0" in err()
    assert lib.ccedit_mask_composite_graded(P, P, P, P, 1, 0, None) == -1 and b"P=0" in err()
    assert lib.ccedit_inpaint_blend_level(None, P, P, P, P, 1, 4, 64, 128, 1.0, 1.5, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_inpaint_blend_level(P, P, P, None, P, 1, 4, 64, 128, 1.0, 1.5, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_inpaint_blend_level(P, P, P, P, P, 1, 4, 64, 0, 1.0, 1.5, None) == -1 and b"thr=0" in err()
    assert lib.ccedit_inpaint_blend_level(P, P, P, P, P, 1, 4, 64, 256, 1.0, 1.5, None) == -1 and b"thr=256" in err()
    assert lib.ccedit_inpaint_blend_level(P, P, P, P, P, 1, 0, 64, 128, 1.0, 1.5, None) == -1 and b"C=0" in err()
    assert lib.ccedit_inpaint_blend_level(P, P, P, P, P, 1, 4, 64, 128, 1.0, 0.0, None) == -1 and b"must be positive" in err()
    from ccedit_amd import ops
    import torch
    with pytest.raises(ValueError, match=r"0 \.\.\. 64"):
        ops.mask_feather(torch.zeros(1, 8, 8, dtype=torch.uint8), 65)
    with pytest.raises(ValueError, match=r"1 \.\.\. 255"):
        ops.inpaint_blend_level(None, None, None, None, 0, 1.0, 1.5)
    m = torch.zeros(1, 8, 8, dtype=torch.uint8)
    assert ops.mask_feather(m, 0) is m                                         # radius 0: the map itself, nothing launched
