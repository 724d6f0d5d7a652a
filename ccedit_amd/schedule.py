"""Prompt schedules: a prompt per time span of a clip (`--prompt_at INDEX:TEXT`, `--prompt_ease`), "prompt travel".

The text enters the network only in the spatial transformers' cross-attention, which is evaluated per frame (the temporal layers of the
shipped configs have no text attention).  So a prompt that changes over the keyframes costs ONE network evaluation, with a text context
per frame: `cond["crossattn"]` of shape (B*T, L, C) instead of (B, L, C) (ccedit_amd/network.py: context_per_frame).

Host side, no device needed:
  parse(entries, num_frames)      "INDEX:TEXT" strings -> [(keyframe index, text)] sorted by index; refusals name the flag
  distinct(base, keyed)           the P distinct texts of a schedule and [(keyframe index, text id)], the base prompt holding from frame 0
  plan(keys, num_frames, ease)    the per-frame table: int32 k0[N], k1[N] (text ids) and float32 a[N]
Device side:
  contexts(c, table)              ops.prompt_schedule (csrc/prompt.hip): fp32 (P, L, C) + table -> fp32 (N, L, C), bit-equal to
                                  tests/_schedule_numpy.py, which imports `plan` from here: the table is data on both sides
  conditioning(...)               the (c, uc) pair of one clip, both made ONCE per clip as stable tensors: the wrapper's per-clip caches
                                  (tensor_key, PinnedCache, the captured graphs) see the same objects at every evaluation.

Between two keyed frames f0 < f1 the context moves from prompt(f0) to prompt(f1) by a(f):
  linear   a = (f - f0) / (f1 - f0)
  smooth   a^2 (3 - 2 a) of the linear a
  step     0 before the midpoint, 1 from it on
all in float32, every operation rounded.  At a keyed frame a is exactly 0 (the frame opens its own span); before the first keyed frame the
first prompt holds, after the last keyed frame the last one: k0 == k1, a == 0.  Image quality is not claimed: what a context between two
prompts makes the network draw is the network's business.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

EASES = ("linear", "smooth", "step")
FLAG = "--prompt_at"


def parse(entries: Sequence[str], num_frames: int) -> List[Tuple[int, str]]:
    """`--prompt_at` values -> [(index, text)] sorted by index.  INDEX is a keyframe index 0 ... N-1, negative values count from the end;
    everything after the FIRST colon is the text."""
    n = int(num_frames)
    if n < 1:
        raise ValueError(f"{FLAG}: a clip of {n} keyframes")
    out, seen = [], {}
    for e in entries:
        head, sep, text = str(e).partition(":")
        if not sep:
            raise ValueError(f"{FLAG} {e!r}: expected INDEX:TEXT")
        try:
            idx = int(head.strip())
        except ValueError:
            raise ValueError(f"{FLAG} {e!r}: INDEX {head!r} is not an integer") from None
        if not -n <= idx < n:
            raise ValueError(f"{FLAG} {e!r}: index {idx} is outside the clip's {n} keyframes ({-n} ... {n - 1})")
        if not text.strip():
            raise ValueError(f"{FLAG} {e!r}: the text is empty")
        f = idx % n
        if f in seen:
            raise ValueError(f"{FLAG} {e!r}: keyframe {f} is keyed twice (also by {seen[f]!r})")
        seen[f] = str(e)
        out.append((f, text))
    return sorted(out, key=lambda p: p[0])


def distinct(base: str, keyed: Sequence[Tuple[int, str]]) -> Tuple[List[str], List[Tuple[int, int]]]:
    """(texts, keys): the distinct texts in order of first use and [(keyframe index, id into texts)].  `base` (--prompt) holds from
    keyframe 0 up to the first keyed index unless index 0 is keyed itself."""
    sched = list(keyed)
    if not sched or sched[0][0] != 0:
        sched = [(0, base)] + sched
    texts: List[str] = []
    keys = []
    for f, t in sched:
        if t not in texts:
            texts.append(t)
        keys.append((int(f), texts.index(t)))
    return texts, keys


def plan(keys: Sequence[Tuple[int, int]], num_frames: int, ease: str = "linear"):
    """keys [(keyframe index, text id)], indices strictly increasing inside 0 ... N-1 -> (k0 int32 [N], k1 int32 [N], a float32 [N])."""
    if ease not in EASES:
        raise ValueError(f"--prompt_ease {ease!r}: one of {', '.join(EASES)}")
    n = int(num_frames)
    keys = [(int(f), int(k)) for f, k in keys]
    if n < 1 or not keys:
        raise ValueError(f"plan: {len(keys)} keyed frames for a clip of {n} keyframes")
    if any(not 0 <= f < n for f, _ in keys) or any(b[0] <= a_[0] for a_, b in zip(keys, keys[1:])) or any(k < 0 for _, k in keys):
        raise ValueError(f"plan: keyed indices {[f for f, _ in keys]} must increase strictly inside 0 ... {n - 1}, text ids must not be negative")
    k0, k1, a = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32)
    one, two, three = np.float32(1), np.float32(2), np.float32(3)
    for f in range(n):
        j = max([i for i, (kf, _) in enumerate(keys) if kf <= f], default=-1)
        if j < 0:                                       # before the first keyed frame: it holds
            k0[f] = k1[f] = keys[0][1]
        elif j == len(keys) - 1:                        # from the last keyed frame on: it holds
            k0[f] = k1[f] = keys[j][1]
        else:
            (f0, p0), (f1, p1) = keys[j], keys[j + 1]
            k0[f], k1[f] = p0, p1
            if p0 != p1:                                # (a span between two equal texts has nowhere to move)
                lin = np.float32(np.float32(f - f0) / np.float32(f1 - f0))
                if ease == "linear":
                    a[f] = lin
                elif ease == "smooth":
                    a[f] = np.float32(np.float32(lin * lin) * np.float32(three - np.float32(two * lin)))
                else:
                    a[f] = one if lin >= np.float32(0.5) else np.float32(0)
    return k0, k1, a


def table_log(keys, k0, k1, a, ease: str) -> dict:
    """log_info.json `prompt_schedule`."""
    return dict(keyed=[int(f) for f, _ in keys], ease=ease, frames=[[int(x), int(y), float(z)] for x, y, z in zip(k0, k1, a)])


def contexts(c, table):
    """fp32 (P, L, C) on the device, (k0, k1, a) -> fp32 (N, L, C): one launch of ccedit_prompt_schedule."""
    from . import ops
    return ops.prompt_schedule(c.float().contiguous(), *table)


def conditioning(c_texts, uc_text, table):
    """The per-frame crossattn pair of ONE clip: c_texts fp32 (P, L, C) (the encoded distinct prompts), uc_text (1, L, C) (the negative
    prompt, which is not scheduled) -> (c (N, L, C), uc (N, L, C)), both new contiguous tensors made once."""
    if uc_text.shape[0] != 1 or tuple(uc_text.shape[1:]) != tuple(c_texts.shape[1:]):
        raise ValueError(f"prompt schedule: negative context {tuple(uc_text.shape)} against {tuple(c_texts.shape)}: one clip, one length")
    n = len(table[0])
    return contexts(c_texts, table), uc_text.float().expand(n, -1, -1).contiguous()
