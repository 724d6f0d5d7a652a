"""The emphasis rule of weighted prompts, restated in numpy: what csrc/prompt.hip must reproduce bit for bit (nothing here imports the
product)."""
import numpy as np

CHUNK = 77


def prompt_weight(z: np.ndarray, e: np.ndarray, w: np.ndarray) -> np.ndarray:
    """z float32 (B, 77 n, C), e float32 (77, C) the empty chunk's encoding, w float32 (B, 77 n) -> float32 (B, 77 n, C):
    out[b, t] = e[t mod 77] + w[b, t] * (z[b, t] - e[t mod 77]) — one float32 subtract, one multiply, one add, each rounded, in that
    order; a row with w == 1 is a copy of z's bits (e + (z - e) is not z in floating point)."""
    assert z.dtype == np.float32 and e.dtype == np.float32 and w.dtype == np.float32
    b, l, c = z.shape
    assert l % CHUNK == 0 and e.shape == (CHUNK, c) and w.shape == (b, l)
    et = e[np.arange(l) % CHUNK][None]                                 # (1, L, C)
    with np.errstate(all="ignore"):
        d = (z - et).astype(np.float32)
        m = (w[:, :, None] * d).astype(np.float32)
        out = (et + m).astype(np.float32)
    return np.where((w == np.float32(1.0))[:, :, None], z, out)
