"""A float64 reference of ccedit_attention that INTERPRETS the descriptor (helper of tests/test_attn_ref.py and
tests/test_attn_desc_gpu.py; no tests in here).

The per-layout references of tests/test_ops_gpu.py rebuild each layout by a reshape / permute written for that layout.  This one
takes the flat 2-D buffers and the keywords of `ops.attention` and restates the address rules of include/ccedit_hip.h (CcAttnDesc)
and ccedit_amd/csrc/attention.hip literally, one row index at a time:

    q row of (batch, i)   = (batch // q_inner) * q_outer_rows + (batch % q_inner) * q_inner_rows + i * q_seq_rows
    kv batch              = batch // kv_div, rows by the same form with the kv fields
    keys [0, seg1_len)    come from kv batch (batch // seg1_div) * seg1_mul + seg1_add, keys [seg1_len, Lk) from the own kv batch
                            at key - seg1_len
    head h                = columns [h * d, (h + 1) * d) of each view
    causal                = key j is visible to query i iff j <= i
    q_log2                = scores are q.k * ln 2 (q arrives in log2 units), no d^-0.5
    scale                 = scores are q.k * scale; None: d^-0.5 (ignored with q_log2)

`Rules` holds exactly these; tests/test_attn_ref.py derives classes from it that make one mistake each, to show that the cases of
tests/test_attn_desc_gpu.py would notice it.
"""
import math

import torch

_DEFAULTS = dict(q_inner=1, q_outer_rows=None, q_inner_rows=0, q_seq_rows=1, kv_div=1, kv_inner=1, kv_outer_rows=None,
                 kv_inner_rows=0, kv_seq_rows=1, out=None, seg1_len=0, seg1_div=1, seg1_mul=0, seg1_add=0, causal=False,
                 q_log2=False, scale=None)


class Rules:
    """The address and score rules of one launch.  Every method is one line of the header's contract."""

    def __init__(self, heads, d, *, batches, lq, lk, **kw):
        unknown = set(kw) - set(_DEFAULTS)
        assert not unknown, f"not keywords of ops.attention: {sorted(unknown)}"
        self.heads, self.d, self.batches, self.lq, self.lk = heads, d, batches, lq, lk
        for name, default in _DEFAULTS.items():
            setattr(self, name, kw.get(name, default))
        if self.q_outer_rows is None:
            self.q_outer_rows = lq                    # as ops.attention fills them in
        if self.kv_outer_rows is None:
            self.kv_outer_rows = lk
        assert 0 <= self.seg1_len <= lk and (not self.causal or (lq == lk and self.seg1_len == 0))

    # ---- rows ----
    def q_row(self, batch, i):
        return (batch // self.q_inner) * self.q_outer_rows + (batch % self.q_inner) * self.q_inner_rows + i * self.q_seq_rows

    def kv_base(self, kvb):
        return (kvb // self.kv_inner) * self.kv_outer_rows + (kvb % self.kv_inner) * self.kv_inner_rows

    def kv_batch(self, batch):
        return batch // self.kv_div

    def seg1_batch(self, batch):
        return (batch // self.seg1_div) * self.seg1_mul + self.seg1_add

    def kv_row(self, batch, j):
        if j < self.seg1_len:
            return self.kv_base(self.seg1_batch(batch)) + j * self.kv_seq_rows
        return self.kv_base(self.kv_batch(batch)) + (j - self.seg1_len) * self.kv_seq_rows

    # ---- columns ----
    def head_col(self, h):
        return h * self.d

    # ---- element access: [len(rows), d] of head h (a method so that a mistake may address outside the view) ----
    def gather(self, t, rows, h):
        c0 = self.head_col(h)
        assert 0 <= c0 and c0 + self.d <= t.shape[1] and min(rows) >= 0 and max(rows) < t.shape[0], "descriptor addresses outside the view"
        return t[torch.tensor(rows), c0:c0 + self.d]

    # ---- scores ----
    def score_scale(self):
        if self.q_log2:
            return math.log(2.0)
        return float(self.d) ** -0.5 if self.scale is None else float(self.scale)

    def visible(self, i, j):
        return (not self.causal) or j <= i

    def q_rows(self, batch):
        return [self.q_row(batch, i) for i in range(self.lq)]

    def kv_rows(self, batch):
        return [self.kv_row(batch, j) for j in range(self.lk)]


def _out_shape(q2d, r):
    return tuple(r.out.shape) if r.out is not None else (q2d.shape[0], r.heads * r.d)


def attn_ref(q2d, k2d, v2d, heads, d, rules=Rules, **desc):
    """(out64, written): the float64 result placed in a zero buffer of the shape of `out` (default [q rows, heads * d], as
    ops.attention allocates it), and the boolean mask of the output elements the descriptor addresses.  q2d / k2d / v2d: the CPU
    views that ops.attention would be handed on the device."""
    r = rules(heads, d, **desc)
    out = torch.zeros(_out_shape(q2d, r), dtype=torch.float64)
    written = torch.zeros(out.shape, dtype=torch.bool)
    if r.causal:
        vis = torch.tensor([[r.visible(i, j) for j in range(r.lk)] for i in range(r.lq)])
    for batch in range(r.batches):
        qr, kr = r.q_rows(batch), r.kv_rows(batch)
        for h in range(heads):
            q, k, v = r.gather(q2d, qr, h).double(), r.gather(k2d, kr, h).double(), r.gather(v2d, kr, h).double()
            s = (q @ k.T) * r.score_scale()
            if r.causal:
                s = s.masked_fill(~vis, -math.inf)
            p = torch.exp(s - s.max(dim=1, keepdim=True).values)
            o = (p @ v) / p.sum(dim=1, keepdim=True)
            c0 = Rules.head_col(r, h)                  # the output is always placed by the true rule
            rows = torch.tensor([Rules.q_row(r, batch, i) for i in range(r.lq)])
            assert not written[rows, c0:c0 + d].any(), "two (batch, head, query) write one output element"
            out[rows, c0:c0 + d] = o
            written[rows, c0:c0 + d] = True
    return out, written


def attn_read_masks(q_shape, k_shape, v_shape, heads, d, rules=Rules, **desc):
    """(mq, mk, mv): boolean masks, in the shapes of the three views, of the elements the descriptor reads."""
    r = rules(heads, d, **desc)
    mq, mk, mv = (torch.zeros(tuple(s), dtype=torch.bool) for s in (q_shape, k_shape, v_shape))
    for batch in range(r.batches):
        qr, kr = torch.tensor(r.q_rows(batch)), torch.tensor(r.kv_rows(batch))
        assert qr.min() >= 0 and qr.max() < mq.shape[0] and kr.min() >= 0 and kr.max() < min(mk.shape[0], mv.shape[0])
        for h in range(heads):
            c0 = r.head_col(h)
            assert c0 + d <= min(mq.shape[1], mk.shape[1], mv.shape[1])
            mq[qr, c0:c0 + d] = True
            mk[kr, c0:c0 + d] = True
            mv[kr, c0:c0 + d] = True
    return mq, mk, mv
