"""The quality report (`--report_quality`), the parts that can be checked without a GPU: the numpy restatement
(tests/_quality_numpy.py) against hand-computed values and against the properties that make it worth matching, the host logic of
ccedit_amd/quality.py (constants, what is derived from the integers), the command-line surface, and the two C-ABI entry points:
declared, exported, bound, arguments validated before any HIP call.

The bounds on the two scenes are the issue's: the inverse of a clip has exactly the clip's own warp sums, a clip that flickers by +-12
grey levels has at least 10 x the source's warp error (the restatement gives 48 x at 64 x 128 and 93 x at 128 x 192, printed), and the
matcher follows at least 0.9 of the pixels (0.963 and 0.978)."""
import ctypes
import functools
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _quality_numpy as ref  # noqa: E402
from _masktrack_scenes import scene  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ("ccedit_quality_pair", "ccedit_quality_warp")


@functools.lru_cache(maxsize=None)
def _scene(h, w):
    """(clip, pair rows, per-pixel vectors) of scene(h, w, 5, seed=3) — computed once, shared and never written to."""
    clip = scene(h, w, 5, seed=3, bg=(1, -2), obj=(-2, 3))[0]
    rows, vsel = ref.fields(clip)
    for a in (clip, rows, vsel):
        a.setflags(write=False)
    return clip, rows, vsel


def _rand(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


# ---- 1. constants and host arithmetic ---------------------------------------------------------------
def test_the_constants_are_the_same_in_the_module_and_in_the_restatement():
    from ccedit_amd import masktrack, quality
    for name in ("WINDOW", "STRIDE", "C1", "C2", "Q_ONE", "KEEP_BELOW", "FB_LIMIT", "PAIR_CHUNK"):
        assert getattr(quality, name) == getattr(ref, name), name
    assert quality.C1 == round((0.01 * 255) ** 2 * quality.WINDOW ** 4) and quality.C2 == round((0.03 * 255) ** 2 * quality.WINDOW ** 4)
    assert quality.Q_ONE == 2 ** 32 and quality.FB_LIMIT == masktrack.FB_LIMIT == 1 and quality.PAIR_CHUNK % 2 == 0
    assert np.array_equal(quality.pair_rows(5, 0), ref.pair_rows(5))
    src = open(os.path.join(ROOT, "ccedit_amd", "csrc", "quality.hip")).read()
    assert f"kC1 = {quality.C1};" in src and f"kC2 = {quality.C2};" in src


def test_derive_compare_and_derive_temporal_equal_the_restatement_and_guard_every_division():
    from ccedit_amd import quality
    rows = [[10, 20, 30, 64, 5 * 2 ** 31, 3, 6400, 6464], [0, 0, 0, 0, 0, 0, 0, 0], [1, 2, 3, 64, -2 ** 30, 1, 640, 0]]
    d = quality.derive_compare(rows)
    assert d == ref.derive_compare(rows)
    assert d["sse"] == [11, 22, 33] and d["count"] == 128 and d["windows"] == 4 and not d["identical"]
    assert d["psnr"] == pytest.approx(10 * math.log10(65025 * 3 * 128 / 66), rel=1e-12)
    assert d["ssim"] == pytest.approx((5 * 2 ** 31 - 2 ** 30) / (4 * 2 ** 32), rel=1e-12)
    assert d["mean_luma_a"] == [100.0, None, 10.0] and d["flicker"] == {"a": None, "b": None}
    none = quality.derive_compare([[0] * 8])
    assert none["psnr"] is None and none["ssim"] is None and none["identical"] is False and none["psnr_rgb"] == [None] * 3
    same = quality.derive_compare([[0, 0, 0, 64, 2 ** 32, 1, 64, 64], [0, 0, 0, 64, 2 ** 32, 1, 128, 192]])
    assert same["identical"] is True and same["psnr"] is None and same["ssim"] == 1.0 and same["flicker"] == {"a": 1.0, "b": 2.0}
    t = quality.derive_temporal([(1, 0), (2, 1)], [[30, 60, 5, 8], [0, 0, 0, 8]], True)
    assert (t["warp_mse"], t["warp_mse_y"], t["valid_share"]) == (2.0, 4.0, 5 / 16) and t["pairs"] == [[1, 0], [2, 1]]
    t = quality.derive_temporal([(1, 0)], [[0, 0, 0, 0]], False)
    assert (t["warp_mse"], t["warp_mse_y"], t["valid_share"], t["sse_y"]) == (None, None, None, None)


def test_the_host_functions_refuse_what_is_not_a_clip_on_the_device():
    import torch
    from ccedit_amd import quality
    cpu = torch.zeros((2, 64, 64, 3), dtype=torch.uint8)
    for call in (lambda: quality.compare(cpu, cpu), lambda: quality.temporal(cpu, cpu), lambda: quality.report(cpu, cpu)):
        with pytest.raises(ValueError, match="cuda uint8"):
            call()
    with pytest.raises(ValueError, match="at least 2"):
        quality.check_temporal(1, 64, 64)
    with pytest.raises(ValueError, match="multiples of 64"):
        quality.check_temporal(5, 72, 64)
    quality.check_temporal(2, 64, 128)


# ---- 2. the restatement: fidelity ---------------------------------------------------------------------
def test_a_hand_computed_window():
    """8 x 8, one window.  a: grey 100 everywhere; b: grey 100 on the left half, 120 on the right half.  Grey means luma = the value:
    (256 v + 128) >> 8 = v."""
    a = np.full((8, 8, 3), 100, np.uint8)
    b = a.copy()
    b[:, 4:] = 120
    s1, s2 = 64 * 100, 32 * 100 + 32 * 120
    saa, sbb, sab = 64 * 100 ** 2, 32 * 100 ** 2 + 32 * 120 ** 2, 32 * 100 * 100 + 32 * 100 * 120
    assert (s1, s2, saa, sbb, sab) == (6400, 7040, 640000, 780800, 704000)
    va, vb, cov = 64 * saa - s1 ** 2, 64 * sbb - s2 ** 2, 64 * sab - s1 * s2
    assert (va, vb, cov) == (0, 409600, 0)
    nw, dw = (2 * s1 * s2 + 26634) * (2 * cov + 239708), (s1 ** 2 + s2 ** 2 + 26634) * (va + vb + 239708)
    assert (nw, dw) == (90138634 * 239708, 90548234 * 649308)
    q = (nw << 32) // dw
    got = ref.pair_frame(a, b)
    assert got == [32 * 400, 32 * 400, 32 * 400, 64, q, 1, 6400, 7040]
    assert q == 1578420176 and 0 < q < 2 ** 32            # 0.36750 of one: the means nearly agree, the variances do not
    nwa, dwa = ref.window_terms(ref.luma(a), ref.luma(b))
    assert (int(nwa[0, 0]), int(dwa[0, 0])) == (nw, dw)
    assert ref.quotient(-nw, dw) == -q and ref.quotient(0, dw) == 0 and ref.quotient(dw, dw) == 2 ** 32


@pytest.mark.parametrize("h,w", [(8, 8), (12, 20), (64, 64), (72, 136)])
def test_identical_frames_have_no_error_and_full_quotients(h, w):
    a = _rand((2, h, w, 3), h)
    windows = ((h - 8) // 4 + 1) * ((w - 8) // 4 + 1)
    for row in ref.pair(a, a):
        assert row[:6] == [0, 0, 0, h * w, windows * 2 ** 32, windows] and row[6] == row[7]


def test_the_measure_is_symmetric_and_a_uniform_shift_gives_d_squared_per_pixel():
    a, b = _rand((1, 24, 36, 3), 1), _rand((1, 24, 36, 3), 2)
    m = (_rand((1, 24, 36), 3) > 200).astype(np.uint8) * 255
    for mask in (None, m):
        ab, ba = ref.pair(a, b, mask)[0], ref.pair(b, a, mask)[0]
        assert ab[:6] == ba[:6] and (ab[6], ab[7]) == (ba[7], ba[6])
    low = (a >> 1).astype(np.uint8)                        # <= 127: + 100 stays a byte
    d = 100
    row = ref.pair(low, (low + d).astype(np.uint8), m)[0]
    kept = int((m < 128).sum())
    assert row[:4] == [d * d * kept] * 3 + [kept] and row[7] - row[6] == d * kept      # luma(v + d) = luma(v) + d: the weights sum to 256


def test_masks_choose_the_pixels_and_only_whole_windows_count():
    a, b = _rand((1, 16, 16, 3), 4), _rand((1, 16, 16, 3), 5)
    none = np.full((1, 16, 16), 255, np.uint8)
    assert ref.pair(a, b, none)[0] == [0] * 8
    assert ref.pair(a, b, np.zeros((1, 16, 16), np.uint8)) == ref.pair(a, b) == ref.pair(a, b, np.full((1, 16, 16), 127, np.uint8))
    one = none.copy()
    one[0, 4:12, 8:16] = 0                                 # exactly the window at (4, 8)
    row = ref.pair(a, b, one)[0]
    assert row[3] == 64 and row[5] == 1
    assert row[:3] + row[4:] == (lambda r: r[:3] + r[4:])(ref.pair_frame(a[0, 4:12, 8:16], b[0, 4:12, 8:16]))
    one[0, 7, 11] = 128                                    # one pixel of it edited: no window is whole
    assert ref.pair(a, b, one)[0][3:6] == [63, 0, 0]


def test_the_products_stay_inside_63_bits_at_the_extremes():
    z, o = np.zeros((8, 8), np.uint8), np.full((8, 8), 255, np.uint8)
    chk = (np.indices((8, 8)).sum(0) % 2 * 255).astype(np.uint8)
    half = np.where(np.arange(8)[None, :] < 4, 0, 255).astype(np.uint8).repeat(8, 0).reshape(8, 8)
    worst = 0
    for ya in (z, o, chk, 255 - chk, half, 255 - half):
        for yb in (z, o, chk, 255 - chk, half, 255 - half):
            nw, dw = (int(v[0, 0]) for v in ref.window_terms(ya, yb))
            assert 0 < dw < 2 ** 63 and abs(nw) <= dw
            assert -2 ** 32 <= ref.quotient(nw, dw) <= 2 ** 32
            worst = max(worst, dw)
    print("largest Dw:", worst)
    assert worst < 3 * 10 ** 17                            # (the issue's bound: about 2.8e17)
    nw, dw = (int(v[0, 0]) for v in ref.window_terms(chk, 255 - chk))
    assert nw < 0 and ref.quotient(nw, dw) < 0             # opposite checkerboards: negative covariance
    assert ref.quotient(*(int(v[0, 0]) for v in ref.window_terms(o, o))) == 2 ** 32


# ---- 3. the restatement: warp error on the two scenes ----------------------------------------------------
def test_the_first_pair_of_the_small_scene_has_the_sums_the_issue_states():
    clip, rows, vsel = _scene(64, 128)
    assert ref.warp(clip, None, vsel[:2], rows[:2])[0] == [315593, 0, 7895, 8192]


@pytest.mark.parametrize("h,w,share", [(64, 128, 0.963), (128, 192, 0.978)])
def test_inverse_equals_source_and_flicker_is_far_above_it(h, w, share):
    clip, rows, vsel = _scene(h, w)
    sums = ref.warp(clip, 255 - clip, vsel, rows)
    assert all(r[0] == r[1] for r in sums), "255 - source must have exactly the source's sums"
    flick = (255 - clip).astype(np.int32) + np.where(np.arange(5) % 2 == 0, 12, -12)[:, None, None, None]
    flick = np.clip(flick, 0, 255).astype(np.uint8)
    f = ref.warp(flick, None, vsel, rows)
    assert [r[2:] for r in f] == [r[2:] for r in sums]      # the same vectors: the same pixels
    s, fl, vs = ref.warp_mse(sums), ref.warp_mse(f), ref.valid_share(sums)
    print(f"{h}x{w}: source {s:.2f} flicker {fl:.1f} ratio {fl / s:.1f} valid share {vs:.3f}")
    assert fl >= 10 * s and vs >= 0.9
    assert vs == pytest.approx(share, abs=5e-4)


def test_selections_split_the_pixels_and_out_of_range_rows_are_clamped():
    clip, rows, vsel = _scene(64, 128)
    mask = np.where(np.arange(128)[None, None, :] < 40, 255, 0).astype(np.uint8).repeat(64, 1).repeat(5, 0)
    every, edited, kept = (ref.warp(clip, 255 - clip, vsel, rows, mask, sel=s) for s in (0, 1, 2))
    for e, a, b in zip(every, edited, kept):
        assert e == [x + y for x, y in zip(a, b)]
    wild = rows.copy()
    wild[0, :2], wild[2, :2] = (99, -5), (-1, 4)
    assert ref.warp(clip, None, vsel, wild)[:2] == ref.warp(clip, None, vsel, np.array([[4, 0, 0, 0], [0, 0, 0, 0], [0, 4, 0, 0], [0, 0, 0, 0]]))


def test_report_has_no_temporal_part_for_one_frame_or_off_the_grid():
    clip = _scene(64, 128)[0]
    assert ref.report(clip[:1], clip[:1])["temporal"] is None
    assert ref.report(clip[:, :56], clip[:, :56])["temporal"] is None
    rep = ref.report(clip, 255 - clip)
    assert rep["temporal"]["all"]["ratio"] == 1.0 and set(rep["temporal"]) == {"all"} and rep["fidelity"]["ssim"] < 0.5


# ---- 4. the command line -----------------------------------------------------------------------------
JOB = ["--prompt", "a red fox", "--video_path", "clip.gif", "--H", "64", "--W", "128"]


def test_both_entry_points_accept_the_flag_and_refuse_bad_combinations(monkeypatch):
    from scripts.sampling import sampling_tv2v as S
    from scripts.sampling import sampling_tv2v_ref as R
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for mod in (S, R):
        assert mod.parse_args([]).report_quality is False
        a = mod.parse_args(["--report_quality"] + JOB)
        assert a.report_quality is True and S.report_quality_on(a)
        assert mod.parse_args(["--report_quality", "--gpu_io", "--save_type", "png", "--propagate"] + JOB).report_quality is True
        with pytest.raises(ValueError, match="give --prompt with --video_path"):
            mod.parse_args(["--report_quality", "--H", "64", "--W", "128"])
        for size in (["--H", "66", "--W", "128"], ["--H", "64", "--W", "4"]):
            with pytest.raises(ValueError, match="multiples of 4"):
                mod.parse_args(["--report_quality", "--prompt", "x", "--video_path", "clip.gif"] + size)
    args = S.parse_args(["--report_quality"] + JOB)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="WORLD_SIZE"):
        S.check_report_quality(args)
    S.check_report_quality(S.parse_args(JOB))               # without the flag nothing is refused


def test_without_the_flag_the_module_is_not_imported():
    code = ("import sys; sys.path.insert(0, %r); from scripts.sampling import sampling_tv2v as S; "
            "a = S.parse_args(['--synthetic', '--video_path', 'clip.gif', '--prompt', 'x', '--H', '64', '--W', '128']); "
            "S.check_report_quality(a); assert not S.report_quality_on(a); print('ccedit_amd.quality' in sys.modules)" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["False"]


def test_the_tools_exist_and_explain_themselves():
    for tool, word in (("quality.py", "--guide"), ("quality_time.py", "--frames")):
        text = open(os.path.join(ROOT, "tools", tool)).read()
        assert word in text and "ccedit_amd" in text
        compile(text, tool, "exec")


# ---- 5. the C ABI ------------------------------------------------------------------------------------
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
    assert len(hip._SIGS["ccedit_quality_pair"][1]) == 8 and len(hip._SIGS["ccedit_quality_warp"][1]) == 13
    for name in ("quality_pair", "quality_warp"):
        assert callable(getattr(ops, name))
    assert "quality.hip" in build.SOURCES and build.EXTRA_FLAGS["quality.hip"] == build.EXTRA_FLAGS["masktrack.hip"]
    assert "-ffp-contract=off" in build.EXTRA_FLAGS["quality.hip"]
    assert lib.ccedit_abi_version() == 12


def test_arguments_are_validated_before_any_hip_call(lib):
    P = 64          # any non-null, 16-byte aligned "pointer": nothing is dereferenced before the checks fail

    def err():
        return lib.ccedit_last_error()
    assert lib.ccedit_quality_pair(None, P, None, P, 1, 8, 8, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_quality_pair(P, P, None, None, 1, 8, 8, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_quality_pair(P, P, None, P, 0, 8, 8, None) == -1 and b"N=0" in err()
    for h, w in ((4, 8), (8, 10), (12, 6), (16388, 8)):
        assert lib.ccedit_quality_pair(P, P, None, P, 1, h, w, None) == -1 and b"multiples of 4" in err()
    assert lib.ccedit_quality_pair(P, P, None, P, 65535, 4096, 4096, None) == -1 and b"2^33" in err()
    assert lib.ccedit_quality_pair(P, P + 2, None, P, 1, 8, 8, None) == -1 and b"aligned" in err()
    assert lib.ccedit_quality_pair(P, P, P + 1, P, 1, 8, 8, None) == -1 and b"aligned" in err()
    assert lib.ccedit_quality_pair(P, P, None, P + 4, 1, 8, 8, None) == -1 and b"aligned" in err()
    ok = (P, None, P, P, None, P, 1, 2, 64, 64, 1, 0, None)

    def warp(**kw):
        names = ("x", "y", "vsel", "pairs", "mask", "acc", "P", "F", "H", "W", "limit", "sel", "stream")
        a = dict(zip(names, ok))
        a.update(kw)
        return lib.ccedit_quality_warp(*[a[n] for n in names])
    assert warp(x=None) == -1 and b"null pointer" in err()
    assert warp(vsel=None) == -1 and b"null pointer" in err()
    assert warp(pairs=None) == -1 and b"null pointer" in err()
    assert warp(acc=None) == -1 and b"null pointer" in err()
    assert warp(P=0) == -1 and b"P=0" in err()
    assert warp(P=32768) == -1 and b"P=32768" in err()
    assert warp(F=0) == -1 and b"F=0" in err()
    assert warp(H=72) == -1 and b"multiples of 64" in err()
    assert warp(W=32) == -1 and b"multiples of 64" in err()
    assert warp(limit=-1) == -1 and b"limit" in err()
    assert warp(sel=3) == -1 and b"sel=3" in err()
    assert warp(sel=-1) == -1 and b"sel=-1" in err()
    assert warp(sel=1) == -1 and b"give one" in err()
    assert warp(sel=2) == -1 and b"give one" in err()
    assert warp(vsel=P + 4) == -1 and b"aligned" in err()
    assert warp(y=P + 2) == -1 and b"aligned" in err()
    assert warp(acc=P + 4) == -1 and b"aligned" in err()
