"""A prompt schedule's per-frame contexts, restated in numpy: what csrc/prompt.hip (ccedit_prompt_schedule) must reproduce bit for bit.
The table (k0, k1, a) comes from ccedit_amd.schedule.plan on both sides: it is data, not part of what is compared."""
import numpy as np

from ccedit_amd.schedule import plan  # noqa: F401  (the one table builder)


def prompt_schedule(c: np.ndarray, k0: np.ndarray, k1: np.ndarray, a: np.ndarray) -> np.ndarray:
    """c float32 (P, L, C), k0 / k1 int (N,), a float32 (N,) -> float32 (N, L, C): out[f] = c[k0[f]] where a[f] == 0, c[k1[f]] where
    a[f] == 1 (copies of the bits), otherwise c[k0] + a (c[k1] - c[k0]) — one float32 subtract, one multiply, one add, each rounded, in
    that order."""
    assert c.dtype == np.float32 and a.dtype == np.float32 and c.ndim == 3
    k0, k1 = np.asarray(k0), np.asarray(k1)
    assert k0.shape == k1.shape == a.shape and k0.ndim == 1
    assert ((k0 >= 0) & (k0 < c.shape[0]) & (k1 >= 0) & (k1 < c.shape[0])).all()
    c0, c1 = c[k0], c[k1]
    av = a[:, None, None]
    with np.errstate(all="ignore"):
        d = (c1 - c0).astype(np.float32)
        m = (av * d).astype(np.float32)
        out = (c0 + m).astype(np.float32)
    out = np.where(av == np.float32(0), c0, out)
    return np.where(av == np.float32(1), c1, out)
