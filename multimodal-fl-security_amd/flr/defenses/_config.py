"""Range checks of the defenses' numeric config fields.  Every message names the
key and shows the offending value."""
from __future__ import annotations

import math
import numbers
from typing import Any, Dict, Optional

import torch


def int_in(cfg: Dict[str, Any], key: str, default: int, lo: int, hi: Optional[int] = None) -> int:
    """cfg[key] (or default): an integer, no bool, in [lo, hi]."""
    v = cfg.get(key, default)
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < lo or (hi is not None and v > hi):
        raise ValueError(f"{key} must be an integer in [{lo}, {'inf' if hi is None else hi}], got {v!r}")
    return int(v)


def real_in(cfg: Dict[str, Any], key: str, default: float, lo: float, hi: Optional[float] = None, *,
            closed: bool = False, finite: bool = True, float32: bool = False, or_else: str = "") -> float:
    """cfg[key] (or default) as a float: a real number, no bool and no NaN,
    above lo (closed: or equal to it), at most hi when one is given, and finite
    unless finite=False.  float32: the kernels take the value as a float32, whose
    rounding must pass the same test (1e-60 rounds to 0, 1e60 to inf).
    or_else: what else the caller accepts for this key, for the message."""
    v = cfg.get(key, default)

    def ok(x: float) -> bool:
        return ((x >= lo if closed else x > lo) and (hi is None or x <= hi)
                and not (finite and math.isinf(x)))

    if isinstance(v, bool) or not isinstance(v, numbers.Real) or math.isnan(v) or not ok(v) \
            or (float32 and not ok(float(torch.tensor(float(v), dtype=torch.float32)))):
        raise ValueError(f"{key} must be a {'finite ' if finite else ''}number {'>=' if closed else '>'} {lo}"
                         f"{'' if hi is None else f' and <= {hi}'}{' (in float32)' if float32 else ''}{or_else}, "
                         f"got {v!r}")
    return float(v)
