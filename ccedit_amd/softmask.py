"""Graded edit masks (`--mask_graded`, `--mask_feather`): the host side — constants, the flag check and the per-step
thresholds.  A strength map is a uint8 pixel map, byte g = edit strength g / 255; its latent strengths L (ops.mask_latent_graded) decide
per sampler step which cells are still held to the noised source: before walked step j of n a cell is free iff L n >= 255 (n - j),
i.e. L >= threshold(j, n).  Kernels: csrc/softmask.hip (feather, latent strengths, composite) and csrc/mask.hip (the re-injection)."""
from __future__ import annotations

from typing import List

FEATHER_MAX = 64          # pixels: a row sum of 2 * 64 + 1 bytes fits the uint16 workspace (129 * 255 = 32 895)


def check_feather(radius) -> int:
    """--mask_feather: 0 ... FEATHER_MAX pixels (ValueError with what to do)."""
    if isinstance(radius, bool) or int(radius) != radius or not 0 <= int(radius) <= FEATHER_MAX:
        raise ValueError(f"--mask_feather {radius}: the feather radius is 0 ... {FEATHER_MAX} pixels (0 = off) — for a wider ramp paint a "
                         "grey mask and give --mask_graded")
    return int(radius)


def threshold(j: int, n: int) -> int:
    """The smallest latent strength that is free (edited, not re-injected) before walked step j of n, j = 0 ... n - 1:
    ceil(255 (n - j) / n).  threshold(0, n) = 255, it never rises with j and never falls below 1."""
    if not (n >= 1 and 0 <= j < n):
        raise ValueError(f"threshold({j}, {n}): step j must be in 0 ... n - 1 of n >= 1 walked steps")
    return (255 * (n - j) + n - 1) // n


def thresholds(n: int) -> List[int]:
    """threshold(j, n) for j = 0 ... n - 1."""
    return [threshold(j, n) for j in range(n)]
