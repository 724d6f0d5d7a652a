"""Prompt schedules without a device: the parser of `--prompt_at` and its refusals, the per-frame table of the three eases, the numpy
restatement's bit-copy rule (tests/_schedule_numpy.py), the new symbol in the header and the binding at ABI 12, and the flag checks of
the entry point."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _schedule_numpy as SN  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(*argv, ref=False):
    from scripts.sampling import sampling_tv2v as S
    from scripts.sampling import sampling_tv2v_ref as R
    return (R if ref else S).parse_args(list(argv))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. the parser -----------------------------------------------------------------------------------
def test_parse_reads_index_and_text_and_sorts():
    from ccedit_amd import schedule
    assert schedule.parse(["3:winter, snow", "-1:night: stars", " 1 : dusk"], 5) == [(1, " dusk"), (3, "winter, snow"), (4, "night: stars")]
    assert schedule.parse(["0:a", "-5:b"][:1], 5) == [(0, "a")]
    assert schedule.parse(["-5:b"], 5) == [(0, "b")]
    assert schedule.parse([], 5) == []


@pytest.mark.parametrize("entries, n, message", [
    (["5:a"], 5, r"--prompt_at '5:a': index 5 is outside the clip's 5 keyframes \(-5 \.\.\. 4\)"),
    (["-6:a"], 5, r"--prompt_at '-6:a': index -6 is outside the clip's 5 keyframes"),
    (["1:a", "-4:b"], 5, r"--prompt_at '-4:b': keyframe 1 is keyed twice \(also by '1:a'\)"),
    (["2:"], 5, r"--prompt_at '2:': the text is empty"),
    (["2:   "], 5, r"the text is empty"),
    (["winter"], 5, r"--prompt_at 'winter': expected INDEX:TEXT"),
    (["x:winter"], 5, r"--prompt_at 'x:winter': INDEX 'x' is not an integer"),
    (["0:a"], 0, r"--prompt_at: a clip of 0 keyframes"),
])
def test_parse_refuses(entries, n, message):
    from ccedit_amd import schedule
    with pytest.raises(ValueError, match=message):
        schedule.parse(entries, n)


def test_distinct_puts_the_base_prompt_first_unless_frame_0_is_keyed():
    from ccedit_amd import schedule
    assert schedule.distinct("summer", [(2, "winter"), (4, "summer")]) == (["summer", "winter"], [(0, 0), (2, 1), (4, 0)])
    assert schedule.distinct("summer", [(0, "spring"), (3, "winter")]) == (["spring", "winter"], [(0, 0), (3, 1)])
    assert schedule.distinct("summer", [(1, "summer"), (3, "summer")]) == (["summer"], [(0, 0), (1, 0), (3, 0)])
    assert schedule.distinct("summer", []) == (["summer"], [(0, 0)])


# ---- 2. the table ------------------------------------------------------------------------------------
def _smooth(a):
    a = np.float32(a)
    return np.float32(np.float32(a * a) * np.float32(np.float32(3) - np.float32(np.float32(2) * a)))


def test_plan_linear_smooth_step_between_two_keys():
    from ccedit_amd import schedule
    keys = [(0, 0), (4, 1)]
    lin = np.array([0, 0.25, 0.5, 0.75, 0], np.float32)
    for ease, want in (("linear", lin), ("smooth", np.array([0, _smooth(0.25), _smooth(0.5), _smooth(0.75), 0], np.float32)),
                       ("step", np.array([0, 0, 1, 1, 0], np.float32))):
        k0, k1, a = schedule.plan(keys, 5, ease)
        assert k0.dtype == np.int32 and k1.dtype == np.int32 and a.dtype == np.float32
        assert k0.tolist() == [0, 0, 0, 0, 1] and k1.tolist() == [1, 1, 1, 1, 1]
        assert np.array_equal(_bits(a), _bits(want)), (ease, a)
    # thirds are rounded once, in float32
    _, _, a = schedule.plan([(0, 0), (3, 1)], 4, "linear")
    assert np.array_equal(_bits(a), _bits(np.array([0, np.float32(1) / np.float32(3), np.float32(2) / np.float32(3), 0], np.float32)))


def test_plan_boundaries():
    from ccedit_amd import schedule
    # keyframe 0 not keyed by the caller: the first key holds before it
    k0, k1, a = schedule.plan([(2, 1), (3, 0)], 5, "linear")
    assert k0.tolist() == [1, 1, 1, 0, 0] and k1.tolist() == [1, 1, 0, 0, 0] and not a.any()
    # last index keyed: it is its own prompt with a == 0; not keyed: the last prompt holds
    k0, k1, a = schedule.plan([(0, 0), (4, 1)], 5, "linear")
    assert (k0[4], k1[4], a[4]) == (1, 1, 0)
    k0, k1, a = schedule.plan([(0, 0), (2, 1)], 5, "linear")
    assert k0.tolist() == [0, 0, 1, 1, 1] and k1.tolist() == [1, 1, 1, 1, 1] and a.tolist() == [0, 0.5, 0, 0, 0]
    # adjacent keyed indices: no frame lies between them
    for ease in schedule.EASES:
        k0, k1, a = schedule.plan([(0, 0), (1, 1), (2, 2)], 3, ease)
        assert k0.tolist() == [0, 1, 2] and not a.any()
    # one frame
    k0, k1, a = schedule.plan([(0, 0)], 1, "smooth")
    assert (k0.tolist(), k1.tolist(), a.tolist()) == ([0], [0], [0.0])
    # a is exactly 0 at every keyed frame and never reaches 1 between two of them except by `step`
    for ease in schedule.EASES:
        keys = [(0, 0), (3, 1), (7, 2), (16, 0)]
        k0, k1, a = schedule.plan(keys, 17, ease)
        assert all(a[f] == 0 and k0[f] == k for f, k in keys)
        assert ((a >= 0) & (a <= 1)).all() and (ease == "step" or (a < 1).all())
        assert set(np.unique(a)) <= {0.0, 1.0} if ease == "step" else True
    # a span between two equal texts does not move
    _, _, a = schedule.plan([(0, 0), (4, 0)], 5, "linear")
    assert not a.any()


def test_plan_step_switches_at_the_midpoint():
    from ccedit_amd import schedule
    _, _, a = schedule.plan([(0, 0), (3, 1)], 4, "step")          # 1/3 -> 0, 2/3 -> 1
    assert a.tolist() == [0, 0, 1, 0]
    _, _, a = schedule.plan([(0, 0), (4, 1)], 5, "step")          # the midpoint itself belongs to the later prompt
    assert a.tolist() == [0, 0, 1, 1, 0]


@pytest.mark.parametrize("keys, n, ease", [([(0, 0)], 3, "cubic"), ([], 3, "linear"), ([(3, 0)], 3, "linear"), ([(1, 0), (1, 1)], 3, "linear"),
                                           ([(2, 0), (1, 1)], 3, "linear"), ([(0, -1)], 3, "linear")])
def test_plan_refuses(keys, n, ease):
    from ccedit_amd import schedule
    with pytest.raises(ValueError):
        schedule.plan(keys, n, ease)


# ---- 3. the numpy restatement ------------------------------------------------------------------------
def test_reference_copies_bits_at_0_and_1_and_rounds_three_times_between():
    rs = np.random.RandomState(3)
    c = rs.randn(3, 4, 6).astype(np.float32)
    c[0, 0, 0], c[1, 0, 0], c[2, 0, 1] = -0.0, 0.0, -0.0
    c[0, 1, 2] = np.float32(np.nan)
    k0, k1 = np.array([0, 0, 1, 2, 0]), np.array([1, 1, 2, 0, 1])
    a = np.array([0, 1, 0.5, 1 / 3, 1], np.float32)
    out = SN.prompt_schedule(c, k0, k1, a)
    assert out.dtype == np.float32 and out.shape == (5, 4, 6)
    assert np.array_equal(_bits(out[0]), _bits(c[0])) and np.array_equal(_bits(out[1]), _bits(c[1])) and np.array_equal(_bits(out[4]), _bits(c[1]))
    assert _bits(out[0])[0, 0] == 0x80000000 and _bits(out[1])[0, 0] == 0          # -0.0 stays -0.0, +0.0 stays +0.0
    for f in (2, 3):
        d = (c[k1[f]] - c[k0[f]]).astype(np.float32)
        want = (c[k0[f]] + (a[f] * d).astype(np.float32)).astype(np.float32)
        assert np.array_equal(_bits(out[f]), _bits(want))
    # c0 + 1 * (c1 - c0) is not c1 in floating point: the copy at a == 1 is a rule, not a consequence
    big = np.array([[[1e8, 1.0]], [[1.0, 1e-8]]], np.float32)
    one = SN.prompt_schedule(big, np.array([0]), np.array([1]), np.array([1], np.float32))
    assert np.array_equal(_bits(one[0]), _bits(big[1]))
    assert (big[0] + (big[1] - big[0]))[0, 1] != big[1][0, 1]
    with pytest.raises(AssertionError):
        SN.prompt_schedule(c, np.array([3]), np.array([0]), np.array([0], np.float32))
    assert SN.plan is __import__("ccedit_amd.schedule", fromlist=["plan"]).plan          # the table is data on both sides


# ---- 4. header, binding, ABI -------------------------------------------------------------------------
def test_the_entry_point_is_declared_bound_and_built_at_abi_12():
    from ccedit_amd import hip
    with open(os.path.join(ROOT, "include", "ccedit_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define CCEDIT_ABI_VERSION 12\b", header) and hip.ABI_VERSION == 12
    assert re.search(r"#define CCEDIT_ATTN_KV_PER_FRAME 2\b", header) and hip.ATTN_KV_PER_FRAME == 2
    assert re.search(r"Prompt schedules \(added without an ABI bump", header)
    assert re.search(r"int ccedit_prompt_schedule\(const float\* c, const int32_t\* k0, const int32_t\* k1, const float\* a, float\* out, int32_t P, "
                     r"int32_t N, int32_t L,\s+int32_t C, void\* stream\);", header)
    assert "ccedit_prompt_schedule" in hip.EXPORTS and len(hip._SIGS["ccedit_prompt_schedule"][1]) == 10
    assert [n for n, _ in hip.CcAttnDesc._fields_][-1] == "flags"
    lib = hip.lib()
    assert lib.ccedit_abi_version() == 12
    import ctypes as C
    k = (C.c_int32 * 2)(0, 2)
    a = (C.c_float * 2)(0.0, 0.5)
    assert lib.ccedit_prompt_schedule(None, k, k, a, None, 2, 2, 77, 768, None) == -1 and b"null pointer" in lib.ccedit_last_error()
    # a bad index is a status, found on the host before anything is launched (the pointers are never followed)
    assert lib.ccedit_prompt_schedule(16, k, k, a, 1 << 40, 2, 2, 77, 768, None) == -1
    assert b"frame 1: k0=2 k1=2 outside the 2 prompts" in lib.ccedit_last_error()
    nan = (C.c_float * 2)(0.0, float("nan"))
    k = (C.c_int32 * 2)(0, 1)
    assert lib.ccedit_prompt_schedule(16, k, k, nan, 1 << 40, 2, 2, 77, 768, None) == -1 and b"frame 1: a=" in lib.ccedit_last_error()
    assert lib.ccedit_prompt_schedule(16, k, k, a, 32, 2, 2, 77, 768, None) == -1 and b"must not alias" in lib.ccedit_last_error()
    assert lib.ccedit_prompt_schedule(16, k, k, a, 1 << 40, 0, 2, 77, 768, None) == -1 and b"positive" in lib.ccedit_last_error()


def test_the_flag_without_kv_div_1_is_refused_by_the_wrapper():
    import torch
    from ccedit_amd import ops
    q = torch.zeros((8, 40), dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="kv_per_frame means one kv batch per batch, got kv_div=2"):
        ops.attention(q, q, q, 1, 40, batches=2, lq=4, lk=4, kv_div=2, kv_per_frame=True)


def test_context_per_frame_shapes():
    import torch
    from ccedit_amd.network import context_per_frame
    assert context_per_frame(torch.zeros(2, 77, 8), 2, 3) is False
    assert context_per_frame(torch.zeros(6, 77, 8), 2, 3) is True
    assert context_per_frame(torch.zeros(2, 77, 8), 2, 1) is False
    for bad in (torch.zeros(3, 77, 8), torch.zeros(12, 77, 8), torch.zeros(6, 8)):
        with pytest.raises(ValueError, match=r"expected \(2, L, C\), one context per clip, or \(6, L, C\), one per frame"):
            context_per_frame(bad, 2, 3)


def test_reserve_windows_sizes_the_text_kv_cache_for_frame_contexts():
    from ccedit_amd.network import OpenAIWrapperControlLDM3DTV2V as W
    w = W.__new__(W)
    w.__dict__["_modules"] = {}
    W.reserve_windows(w, 3)
    assert (w._graph_slots, w._hint_slots, w._tkv_slots) == (3, 6, 6)                     # as before
    W.reserve_windows(w, 5, frame_contexts=True)
    assert (w._graph_slots, w._hint_slots, w._tkv_slots, w._window_contexts) == (5, 10, 10, True)
    W.reserve_windows(w, 0)
    assert (w._graph_slots, w._hint_slots, w._tkv_slots, w._window_contexts) == (2, 4, 6, False)


# ---- 5. the flags ------------------------------------------------------------------------------------
JOB = ("--prompt", "a meadow in summer", "--video_path", "clips/meadow", "--num_keyframes", "5")


def test_flag_defaults_leave_everything_alone():
    from scripts.sampling import sampling_tv2v as S
    for ref in (False, True):
        a = _args(ref=ref)
        assert a.prompt_at is None and a.prompt_ease == "linear" and not S.schedule_on(a)
        S.check_prompt_schedule(a, with_ref=ref)
        S.check_schedule_jobs(a, 7)
    with pytest.raises(SystemExit):
        _args(*JOB, "--prompt_at", "2:winter", "--prompt_ease", "bounce")


def test_flags_give_the_texts_and_the_keys():
    from scripts.sampling import sampling_tv2v as S
    a = _args(*JOB, "--prompt_at", "2:a meadow in winter", "--prompt_at=-1:a meadow at night: stars", "--prompt_ease", "smooth")
    assert S.schedule_on(a) and a.prompt_ease == "smooth"
    assert S.schedule_texts(a) == (["a meadow in summer", "a meadow in winter", "a meadow at night: stars"], [(0, 0), (2, 1), (4, 2)])
    one = _args(*JOB, "--prompt_at", "3:a meadow in summer")
    assert S.schedule_texts(one) == (["a meadow in summer"], [(0, 0), (3, 0)])            # one text: the plain path


@pytest.mark.parametrize("extra, error, message", [
    (("--prompt_at", "5:winter"), ValueError, r"--prompt_at '5:winter': index 5 is outside the clip's 5 keyframes"),
    (("--prompt_at", "1:winter", "--prompt_at=-4:night"), ValueError, r"keyframe 1 is keyed twice"),
    (("--prompt_at", "1:"), ValueError, r"--prompt_at '1:': the text is empty"),
    (("--prompt_at", "1:winter", "--region_prompt", "a bear", "--region_mask", "m.png"), NotImplementedError,
     r"--prompt_at with --region_prompt / --region_mask"),
    (("--prompt_at", "1:winter", "--mask_auto", "--inpainting_mode", "--source_prompt", "a meadow"), NotImplementedError,
     r"--prompt_at with --mask_auto"),
    (("--prompt_at", "1:winter", "--prompt_listpath", "p.txt", "--video_listpath", "v.txt"), ValueError,
     r"--prompt_at schedules the prompts of ONE video: .* --prompt_listpath / --videos_directory / --json_path"),
    (("--prompt_at", "1:winter", "--json_path", "jobs.json"), ValueError, r"--prompt_at schedules the prompts of ONE video"),
])
def test_flag_refusals_come_before_any_video_is_opened(extra, error, message, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    (tmp_path / "m.png").write_bytes(b"")
    with pytest.raises(error, match=message):
        _args(*JOB, *extra)


def test_no_job_and_several_jobs_and_other_gpus_are_refused(monkeypatch):
    from scripts.sampling import sampling_tv2v as S
    with pytest.raises(ValueError, match=r"--prompt_at schedules the prompts of ONE video: give --prompt \(the base prompt\) with --video_path"):
        _args("--num_keyframes", "5", "--prompt_at", "1:winter")
    a = _args(*JOB, "--prompt_at", "1:winter")
    S.check_schedule_jobs(a, 1)
    with pytest.raises(ValueError, match=r"--prompt_at with 3 jobs: a schedule belongs to one video"):
        S.check_schedule_jobs(a, 3)
    a2 = _args(*JOB, "--prompt_at", "1:winter", "--batch_size", "2", "--num_samples", "2")
    with pytest.raises(ValueError, match=r"--prompt_at with --batch_size 2 and 2 clips: .* add --batch_size 1"):
        S.check_schedule_jobs(a2, 1)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match=r"--prompt_at is not available in the multi-GPU modes"):
        S.check_prompt_schedule(a)


def test_the_reference_image_script_refuses_the_flag():
    from scripts.sampling import sampling_tv2v as S
    a = _args(*JOB, "--prompt_at", "1:winter", ref=True)
    with pytest.raises(NotImplementedError, match=r"--prompt_at is not available with a reference image \(sampling_tv2v_ref.py\)"):
        S.check_prompt_schedule(a, with_ref=True)


def test_sharded_wrappers_refuse_a_context_per_frame():
    """_evaluate with a frame shard or a row shard and a (B*T, L, C) context: NotImplementedError before anything is sliced or launched
    (the shard objects are never touched); the (B, L, C) context passes that check and goes on to use the shard."""
    import torch
    from ccedit_amd.network import OpenAIWrapperControlLDM3DTV2V as W
    w = W.__new__(W)
    w.__dict__["_modules"] = {"diffusion_model": None}
    x, t = torch.zeros(2, 4, 3, 8, 8), torch.zeros(2, dtype=torch.int64)
    hint = torch.zeros(2, 3, 3, 64, 64)
    for kw in (dict(frame_shard=object(), row_shard=None), dict(frame_shard=None, row_shard=object())):
        with pytest.raises(NotImplementedError, match="per-frame text context .* not implemented for sharded evaluations"):
            W._evaluate(w, x, t, dict(crossattn=torch.zeros(6, 77, 8), control_hint=hint), half=False, twins=False, **kw)
        with pytest.raises(AttributeError):                  # one context per clip: the check passes, the fake shard is then asked for its geometry
            W._evaluate(w, x, t, dict(crossattn=torch.zeros(2, 77, 8), control_hint=hint), half=False, twins=False, **kw)
