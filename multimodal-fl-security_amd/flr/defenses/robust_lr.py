"""The robust learning rate, RLR (Ozdayi, Kantarcioglu, Gel, "Defending against
Backdoors in Federated Learning with Robust Learning Rate", AAAI 2021).

Per coordinate the clients vote with the sign of their update against the
round's global model g,

  votes[p] = #{k : x_k[p] > g[p]} - #{k : x_k[p] < g[p]}

and where fewer than `threshold` net votes agree, the server's learning rate for
that coordinate is negated:

  out[p] = g[p] + server_lr * (agg[p] - g[p])   |votes[p]| >= threshold
           g[p] - server_lr * (agg[p] - g[p])   otherwise

agg the base rule's aggregate (FedAvg, the median or the trimmed mean).  A
backdoor update survives the row-level rules (Krum, Bulyan, DnC, FoolsGold,
centered clipping) and the trimming ones when its rows lie inside the benign
spread: the harm is done on the few coordinates where the honest clients have no
common opinion and the attackers all push the same way.  There the vote stays
under the threshold and the aggregate moves away from the unopposed minority.
The rule needs no attacker identities and no server data.  The reference
repository has no RLR; tests/robust_lr_ref.py restates the arithmetic of
include/flr.h.

Engine: base "fedavg" is one flr_rlr_fedavg call — the vote rides on the FedAvg
pass, no second pass over the client matrix; the other bases run their own
kernels, then flr_sign_vote and flr_rlr_apply.  Everything is enqueued on the
stream; the votes and the flip count stay on the device until votes() /
get_metrics() ask for them.
"""
from __future__ import annotations

import math
import numbers
from typing import Any, Dict, List, Optional, Sequence, Union

import torch

from .. import ops
from ..matrix import ClientMatrix
from .base_defense import BaseDefense, Updates, as_matrix, source_device
from .trimmed_mean import MedianDefense, TrimmedMeanDefense

DEFAULT_THRESHOLD = 0.25
DEFAULT_SERVER_LR = 1.0
_BASES = {"fedavg": None, "median": MedianDefense, "trimmed_mean": TrimmedMeanDefense}


class RobustLRDefense(BaseDefense):
    """Config: threshold — an int in [0, K] (checked against K at the call), or
    a float in (0, 1) meaning ceil(threshold * K); the default, 0.25, is this
    project's choice (the paper's guidance is only that the threshold must exceed
    the attacker count; the round engine defaults it to min(K, num_attackers +
    1)).  base — "fedavg" (default: the fused kernel), "median" or
    "trimmed_mean", configured by base_cfg.  server_lr — a finite float > 0,
    default 1.0.

    The center of a call (the global model the clients started from), in this
    order: global_flat when given (the round engine's path); the vector of
    set_center(), used by the next call only; this object's own previous result
    when it has the same length; on a first call the coordinate-wise lower median
    of the rows.

    num_examples weighs the FedAvg base only; the vote is one client, one vote."""

    # coordinate-wise: a rank aggregates its coordinate range from the center's
    # slice; the center must line up with the columns, so torch order
    supports_sharded = True
    order_free = False

    def __init__(self, defense_config: Dict[str, Any]):
        super().__init__(defense_config)
        th = defense_config.get("threshold", DEFAULT_THRESHOLD)
        if isinstance(th, bool) or not isinstance(th, numbers.Real) or math.isnan(th):
            raise ValueError(f"threshold must be an integer >= 0 or a float in (0, 1), got {th!r}")
        if isinstance(th, numbers.Integral):
            if th < 0:
                raise ValueError(f"threshold must be an integer >= 0 or a float in (0, 1), got {th!r}")
            self.threshold: Union[int, float] = int(th)
        else:
            if not 0.0 < th < 1.0:
                raise ValueError(f"threshold must be an integer >= 0 or a float in (0, 1), got {th!r}")
            self.threshold = float(th)
        base = defense_config.get("base", "fedavg")
        if not isinstance(base, str) or base not in _BASES:
            raise ValueError(f"base must be one of {', '.join(_BASES)}, got {base!r}")
        self.base = base
        self._base = None if _BASES[base] is None else _BASES[base](dict(defense_config.get("base_cfg") or {}))
        lr = defense_config.get("server_lr", DEFAULT_SERVER_LR)
        if isinstance(lr, bool) or not isinstance(lr, numbers.Real) or not math.isfinite(lr) or lr <= 0 \
                or not 0.0 < float(torch.tensor(float(lr), dtype=torch.float32)) < float("inf"):
            raise ValueError(f"server_lr must be a finite number > 0 (in float32), got {lr!r}")
        self.server_lr = float(lr)
        self._center: Optional[torch.Tensor] = None    # set_center's vector, for the next call
        self._previous: Optional[torch.Tensor] = None  # the last result (a tensor of this object's own)
        self._votes: Optional[torch.Tensor] = None     # device diagnostics of the last call
        self._flipped: Optional[torch.Tensor] = None
        self._theta: Optional[int] = None              # the threshold the last call resolved

    def resolve_threshold(self, K: int) -> int:
        """The vote count a coordinate needs among K clients."""
        if isinstance(self.threshold, int):
            if self.threshold > K:
                raise ValueError(f"threshold {self.threshold} exceeds the {K} clients of this call")
            return self.threshold
        return min(K, math.ceil(self.threshold * K))

    def set_center(self, center: Union[torch.Tensor, Sequence[torch.Tensor], None]) -> None:
        """The global model of the next aggregate call (a flat vector or a
        parameter list, e.g. the initial global model); None withdraws it.  The
        calls after that are centred on their own previous result."""
        if center is None:
            self._center = None
        elif isinstance(center, torch.Tensor):
            self._center = center.detach().reshape(-1).float()
        else:
            self._center = torch.cat([p.detach().reshape(-1).float() for p in center])

    def _start(self, X: torch.Tensor, given: Optional[torch.Tensor]) -> torch.Tensor:
        P = X.shape[1]
        if given is not None:
            if given.numel() != P:
                raise ValueError(f"the center holds {given.numel()} coordinates, the updates {P}")
            return given.detach().reshape(-1).to(device=X.device, dtype=torch.float32).contiguous()
        if self._previous is not None and self._previous.numel() == P and self._previous.device == X.device:
            return self._previous
        return ops.median_lower(X)

    def _rule(self, X: torch.Tensor, num_examples: List[int], g: torch.Tensor, base_aggregate) -> torch.Tensor:
        theta = self.resolve_threshold(X.shape[0])
        if self._base is None:
            out, votes, flipped = ops.rlr_fedavg(X, list(num_examples), g, theta, self.server_lr, diagnostics=True)
        else:
            agg = base_aggregate()
            votes = ops.sign_vote(X, g)
            out, flipped = ops.rlr_apply(agg, g, votes, theta, self.server_lr, out=agg, count=True)
        self._theta, self._votes, self._flipped = theta, votes, flipped
        self._previous = out
        return out

    def aggregate_flat(self, cm: ClientMatrix, num_examples: List[int],
                       global_flat: Optional[torch.Tensor] = None) -> torch.Tensor:
        g = self._start(cm.X, global_flat if global_flat is not None else self._center)
        self._center = None
        return self._rule(cm.X, num_examples, g, lambda: self._base.aggregate_flat(cm, num_examples))

    def aggregate_sharded(self, cs, num_examples: List[int],
                          global_flat: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One rank's coordinate range [cs.begin, cs.end): global_flat is the
        center's slice of that range; set_center's vector is the whole model."""
        given = global_flat
        if given is None and self._center is not None:
            if self._center.numel() != cs.P:
                raise ValueError(f"the center holds {self._center.numel()} coordinates, the updates {cs.P}")
            given = self._center[cs.begin:cs.end]
        g = self._start(cs.X, given)
        self._center = None
        return self._rule(cs.X, num_examples, g, lambda: self._base.aggregate_sharded(cs, num_examples))

    def aggregate(self, client_updates: Updates, num_examples: List[int],
                  global_params: Optional[List[torch.Tensor]] = None) -> List[torch.Tensor]:
        cm = as_matrix(client_updates)
        gflat = None
        if global_params is not None:
            gflat = torch.cat([p.detach().reshape(-1).float() for p in global_params])
        flat = self.aggregate_flat(cm, num_examples, gflat)
        # a copy: the caller may update the returned parameters in place, and
        # the next call is centred on this result
        return cm.unflatten(flat.clone(), source_device(client_updates))

    def votes(self) -> Optional[torch.Tensor]:
        """The last call's votes: a device int32 [P] tensor (None before a call)."""
        return self._votes

    def detect_malicious(self, client_updates: Updates = None, num_examples: List[int] = None) -> List[int]:
        """Always []: the rule judges coordinates, not clients."""
        return []

    def get_metrics(self) -> Dict[str, Any]:
        m = {"defense_type": "robust_lr", "threshold": self.threshold if self._theta is None else self._theta,
             "base": self.base, "server_lr": self.server_lr, "flipped": None, "flipped_fraction": None}
        if self._flipped is not None:
            m["flipped"] = int(self._flipped.item())
            m["flipped_fraction"] = m["flipped"] / self._votes.numel() if self._votes.numel() else 0.0
        return m

    def __repr__(self) -> str:
        return f"RobustLRDefense(threshold={self.threshold}, base={self.base!r}, server_lr={self.server_lr})"
