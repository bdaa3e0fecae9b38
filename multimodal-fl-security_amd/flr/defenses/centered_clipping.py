"""Centered clipping (Karimireddy, He, Jaggi, "Learning from History for
Byzantine Robust Optimization", ICML 2021).

From the previous global model v, `iters` times

  v <- v + (1/K) * sum_i (x_i - v) * min(1, tau / ||x_i - v||)

Every step moves the aggregate by at most tau, so the attackers cannot move it
further than iters * tau however they collude: the defense for ALIE and IPM
(flr.attacks), which stay inside the benign spread that Krum, the trimmed mean,
the median and Bulyan select from.  The client rows are model weights and the
round's global vector is the previous aggregate, exactly the paper's starting
point.  The reference repository has no centered clipping;
tests/centered_clip_ref.py restates the arithmetic of include/flr.h.

Engine: one flr_centered_clip call — per iteration the K distances
(flr_row_norms), the K scales and the combining pass, all enqueued on the
stream with no host round trip; the diagnostics stay on the device until
get_metrics() / detect_malicious() ask for them.
"""
from __future__ import annotations

from typing import Any, Dict, List

import torch

from .. import ops
from ..matrix import ClientMatrix
from ._config import int_in, real_in
from .base_defense import CenteredDefense, Updates

DEFAULT_TAU = 10.0
DEFAULT_ITERS = 3


class CenteredClippingDefense(CenteredDefense):
    """Config: tau — a positive float, or "median": each iteration clips at the
    lower median of its K distances (at most half the rows are clipped, no
    threshold tuned to the model's scale); iters — the number of clipping
    steps.  The defaults, tau = 10.0 and iters = 3, are this project's choice
    (the paper tunes tau per task and runs 1 to 5 steps).

    The clipping starts from the call's center (CenteredDefense).

    num_examples is ignored: the rule is unweighted, as Krum's."""

    # whole rows (the K distances): the engine takes the all-gather exchange, in
    # torch order, and every rank computes the same bits
    supports_sharded = False
    order_free = False

    def __init__(self, defense_config: Dict[str, Any]):
        super().__init__(defense_config)
        if defense_config.get("tau", DEFAULT_TAU) == "median":
            self.tau = 0.0  # flr_centered_clip's adaptive mode
        else:
            self.tau = real_in(defense_config, "tau", DEFAULT_TAU, 0.0, finite=False, float32=True,
                               or_else=" or 'median'")
        self.iters = int_in(defense_config, "iters", DEFAULT_ITERS, 1)
        self._norms = self._scales = self._taus = None  # device diagnostics of the last call

    def _rule(self, cm: ClientMatrix, num_examples: List[int], v0: torch.Tensor) -> torch.Tensor:
        out, self._norms, self._scales, self._taus = ops.centered_clip(cm.X, v0, self.tau, self.iters,
                                                                       diagnostics=True)
        return out

    def detect_malicious(self, client_updates: Updates = None, num_examples: List[int] = None) -> List[int]:
        """The rows clipped (scale < 1) in the last iteration of the last call."""
        if self._scales is None:
            return []
        return torch.nonzero(self._scales[-1] < 1).reshape(-1).cpu().tolist()

    def get_metrics(self) -> Dict[str, Any]:
        m = {"defense_type": "centered_clipping", "tau": "median" if self.tau == 0.0 else self.tau,
             "iters": self.iters, "taus": [], "clipped_counts": [], "final_norms": []}
        if self._scales is not None:
            m["taus"] = self._taus.cpu().tolist()
            m["clipped_counts"] = (self._scales < 1).sum(dim=1).cpu().tolist()
            m["final_norms"] = self._norms[-1].cpu().tolist()
        return m

    def __repr__(self) -> str:
        return f"CenteredClippingDefense(tau={'median' if self.tau == 0.0 else self.tau}, iters={self.iters})"
