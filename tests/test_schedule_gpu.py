"""ccedit_prompt_schedule (csrc/prompt.hip) on a real MI355X: exact, no tolerance, against the numpy restatement of its definition
(tests/_schedule_numpy.py) — vector and scalar paths, a misaligned pointer, a == 0 / 1 as bit copies (signed zeros, NaN payloads), and
a bad index as a status that leaves the output alone."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _schedule_numpy as SN  # noqa: E402

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bits(t):
    a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return a.view(np.uint32)


def _contexts(p, l, c, seed):
    rs = np.random.RandomState(seed)
    x = rs.randn(p, l, c).astype(np.float32)
    x[:, 0, 0] = -0.0                       # signed zeros on both sides of a blend and in the copies
    x[0, 1, 0], x[p - 1, 1, 0] = 0.0, -0.0
    return x


def _table(p, n):
    """Every a of the issue's list — 0, 1, 0.5, 1/3 — over index pairs that cover every prompt, cycled to n frames."""
    avals = [0.0, 1.0, 0.5, np.float32(1) / np.float32(3)]
    k0 = np.array([f % p for f in range(n)], np.int32)
    k1 = np.array([(f + 1) % p for f in range(n)], np.int32)
    a = np.array([avals[(f // 1) % 4] for f in range(n)], np.float32)
    return k0, k1, a


# (P, N, L, C): the issue's shapes; C = 5 takes the one-element path
SHAPES = [(2, 3, 77, 768), (3, 5, 154, 768), (2, 4, 77, 5)]


@pytest.mark.parametrize("p,n,l,c", SHAPES)
def test_prompt_schedule_is_exact(p, n, l, c):
    _need_gpu()
    from ccedit_amd import ops
    x = _contexts(p, l, c, 100 * p + n)
    for shift in range(4):                                                              # every frame meets every a
        k0, k1, a = _table(p, n + shift)
        k0, k1, a = k0[shift:], k1[shift:], a[shift:]
        want = SN.prompt_schedule(x, k0, k1, a)
        xt = torch.from_numpy(x).cuda()
        got = ops.prompt_schedule(xt, k0, k1, a)
        assert got.shape == (n, l, c) and got.dtype == torch.float32
        assert np.array_equal(_bits(got), _bits(want)), f"shift {shift}: {int((_bits(got) != _bits(want)).sum())} elements differ"
        assert np.array_equal(_bits(xt), _bits(x))                                      # the contexts are left alone
        for f in range(n):                                                              # the copies, stated on their own
            if a[f] in (0.0, 1.0):
                assert np.array_equal(_bits(got[f]), _bits(x[k0[f] if a[f] == 0.0 else k1[f]]))


def test_prompt_schedule_from_a_real_plan_and_into_a_given_output():
    _need_gpu()
    from ccedit_amd import ops, schedule
    x = _contexts(3, 77, 768, 7)
    for ease in schedule.EASES:
        k0, k1, a = schedule.plan([(0, 0), (3, 1), (4, 2), (8, 0)], 10, ease)
        out = torch.full((10, 77, 768), 7.0, device="cuda")
        assert ops.prompt_schedule(torch.from_numpy(x).cuda(), k0, k1, a, out=out) is out
        assert np.array_equal(_bits(out), _bits(SN.prompt_schedule(x, k0, k1, a))), ease


def test_prompt_schedule_copies_nan_payloads_and_reads_misaligned_tensors():
    """a == 0 / 1 move bits, whatever they are; tensors 4 bytes off a 16-byte boundary take the one-element accesses."""
    _need_gpu()
    from ccedit_amd import ops
    p, n, l, c = 3, 4, 77, 768
    x = _contexts(p, l, c, 11)
    x.view(np.uint32)[2, 2, :4] = [0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000]      # two NaN payloads, +inf, -inf: in copied frames only
    k0, k1, a = np.array([2, 0, 1, 0], np.int32), np.array([1, 1, 2, 1], np.int32), np.array([0, 0.5, 1, 1 / 3], np.float32)
    want = SN.prompt_schedule(x, k0, k1, a)
    for off_in, off_out in ((1, 0), (0, 3), (2, 1)):
        buf = torch.empty(x.size + 4, dtype=torch.float32, device="cuda")
        xin = buf[off_in:off_in + x.size].view(p, l, c)
        xin.copy_(torch.from_numpy(x))
        obuf = torch.zeros(n * l * c + 4, dtype=torch.float32, device="cuda")
        out = obuf[off_out:off_out + n * l * c].view(n, l, c)
        assert (xin.data_ptr() % 16 == 0) == (off_in == 0) and (out.data_ptr() % 16 == 0) == (off_out == 0)
        ops.prompt_schedule(xin, k0, k1, a, out=out)
        assert np.array_equal(_bits(out), _bits(want)), (off_in, off_out)
        assert _bits(out[0])[2, 0] == 0x7FC00001 and _bits(out[2])[2, 1] == 0xFFC12345
        edge = torch.cat([obuf[:off_out], obuf[off_out + n * l * c:]])
        assert not edge.any(), "elements outside the output were written"


def test_prompt_schedule_more_frames_than_one_launch_takes():
    """The table travels as kernel arguments, 256 frames to a launch: a longer clip is served by further launches."""
    _need_gpu()
    from ccedit_amd import ops
    p, n, l, c = 3, 300, 2, 8
    x = _contexts(p, l, c, 5)
    k0, k1, a = _table(p, n)
    got = ops.prompt_schedule(torch.from_numpy(x).cuda(), k0, k1, a)
    assert np.array_equal(_bits(got), _bits(SN.prompt_schedule(x, k0, k1, a)))


def test_a_bad_index_is_a_status_and_leaves_the_output_untouched():
    _need_gpu()
    from ccedit_amd import hip, ops
    x = torch.from_numpy(_contexts(2, 77, 768, 1)).cuda()
    out = torch.full((3, 77, 768), 5.0, device="cuda")
    ok = np.zeros(3, np.float32)
    for k0, k1, a, message in (([0, 2, 0], [1, 1, 1], ok, "frame 1: k0=2 k1=1 outside the 2 prompts"),
                               ([0, 0, 0], [1, 1, -1], ok, "frame 2: k0=0 k1=-1 outside the 2 prompts"),
                               ([0, 0, 0], [1, 1, 1], np.array([0, 1.5, 0], np.float32), "frame 1: a=1.5"),
                               ([0, 0, 0], [1, 1, 1], np.array([np.nan, 0, 0], np.float32), "frame 0: a=")):
        with pytest.raises(hip.HipLibraryError, match=message):
            ops.prompt_schedule(x, np.array(k0, np.int32), np.array(k1, np.int32), a, out=out)
        torch.cuda.synchronize()
        assert bool((out == 5.0).all()), "a refused call wrote to the output"
    with pytest.raises(hip.HipLibraryError, match="must not alias"):
        ops.prompt_schedule(x, np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(2, np.float32), out=x)
    with pytest.raises(ValueError):
        ops.prompt_schedule(x.double(), np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(2, np.float32))
    with pytest.raises(ValueError):
        ops.prompt_schedule(x, np.zeros(2, np.int32), np.zeros(3, np.int32), np.zeros(2, np.float32))
