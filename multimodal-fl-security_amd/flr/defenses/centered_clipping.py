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

import math
import numbers
from typing import Any, Dict, List, Optional, Sequence, Union

import torch

from .. import ops
from ..matrix import ClientMatrix
from .base_defense import BaseDefense, Updates, as_matrix, source_device

DEFAULT_TAU = 10.0
DEFAULT_ITERS = 3


class CenteredClippingDefense(BaseDefense):
    """Config: tau — a positive float, or "median": each iteration clips at the
    lower median of its K distances (at most half the rows are clipped, no
    threshold tuned to the model's scale); iters — the number of clipping
    steps.  The defaults, tau = 10.0 and iters = 3, are this project's choice
    (the paper tunes tau per task and runs 1 to 5 steps).

    The center of a call, in this order: global_flat when given (the round
    engine's path: the round's global model); the vector of set_center(), used
    by the next call only; this object's own previous result when it has the
    same length (the reference's loop, which passes only the updates: the
    previous result is the global model the clients started from); on a first
    call the coordinate-wise lower median of the rows.

    num_examples is ignored: the rule is unweighted, as Krum's."""

    # whole rows (the K distances): the engine takes the all-gather exchange, in
    # torch order, and every rank computes the same bits
    supports_sharded = False
    order_free = False

    def __init__(self, defense_config: Dict[str, Any]):
        super().__init__(defense_config)
        tau = defense_config.get("tau", DEFAULT_TAU)
        if isinstance(tau, str):
            if tau != "median":
                raise ValueError(f"tau must be a positive number or 'median', got {tau!r}")
            self.tau = 0.0  # flr_centered_clip's adaptive mode
        else:
            if isinstance(tau, bool) or not isinstance(tau, numbers.Real) or math.isnan(tau) or tau <= 0 \
                    or float(torch.tensor(float(tau), dtype=torch.float32)) == 0.0:
                raise ValueError(f"tau must be a positive number (a float32 above 0) or 'median', got {tau!r}")
            self.tau = float(tau)
        iters = defense_config.get("iters", DEFAULT_ITERS)
        if isinstance(iters, bool) or not isinstance(iters, numbers.Integral) or iters < 1:
            raise ValueError(f"iters must be an integer >= 1, got {iters!r}")
        self.iters = int(iters)
        self._center: Optional[torch.Tensor] = None   # set_center's vector, for the next call
        self._previous: Optional[torch.Tensor] = None  # the last result (a tensor of this object's own)
        self._norms = self._scales = self._taus = None  # device diagnostics of the last call

    def set_center(self, center: Union[torch.Tensor, Sequence[torch.Tensor], None]) -> None:
        """The starting point of the next aggregate call (a flat vector or a
        parameter list, e.g. the initial global model); None withdraws it.  The
        calls after that continue from their own previous result."""
        if center is None:
            self._center = None
        elif isinstance(center, torch.Tensor):
            self._center = center.detach().reshape(-1).float()
        else:
            self._center = torch.cat([p.detach().reshape(-1).float() for p in center])

    def _start(self, cm: ClientMatrix, global_flat: Optional[torch.Tensor]) -> torch.Tensor:
        given = global_flat if global_flat is not None else self._center
        if given is not None:
            if given.numel() != cm.P:
                raise ValueError(f"the center holds {given.numel()} coordinates, the updates {cm.P}")
            return given.detach().reshape(-1).to(device=cm.device, dtype=torch.float32).contiguous()
        if self._previous is not None and self._previous.numel() == cm.P and self._previous.device == cm.device:
            return self._previous
        return ops.median_lower(cm.X)

    def aggregate_flat(self, cm: ClientMatrix, num_examples: List[int],
                       global_flat: Optional[torch.Tensor] = None) -> torch.Tensor:
        v0 = self._start(cm, global_flat)
        self._center = None
        out, self._norms, self._scales, self._taus = ops.centered_clip(cm.X, v0, self.tau, self.iters,
                                                                       diagnostics=True)
        self._previous = out
        return out

    def aggregate(self, client_updates: Updates, num_examples: List[int],
                  global_params: Optional[List[torch.Tensor]] = None) -> List[torch.Tensor]:
        cm = as_matrix(client_updates)
        gflat = None
        if global_params is not None:
            gflat = torch.cat([p.detach().reshape(-1).float() for p in global_params])
        flat = self.aggregate_flat(cm, num_examples, gflat)
        # a copy: the caller may update the returned parameters in place, and
        # the next call starts from this result
        return cm.unflatten(flat.clone(), source_device(client_updates))

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
