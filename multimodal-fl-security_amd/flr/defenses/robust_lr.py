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
from typing import Any, Dict, List, Optional, Union

import torch

from .. import ops
from ..matrix import ClientMatrix
from ._config import real_in
from .base_defense import CenteredDefense, Updates
from .trimmed_mean import MedianDefense, TrimmedMeanDefense

DEFAULT_THRESHOLD = 0.25
DEFAULT_SERVER_LR = 1.0
_BASES = {"fedavg": None, "median": MedianDefense, "trimmed_mean": TrimmedMeanDefense}


class RobustLRDefense(CenteredDefense):
    """Config: threshold — an int in [0, K] (checked against K at the call), or
    a float in (0, 1) meaning ceil(threshold * K); the default, 0.25, is this
    project's choice (the paper's guidance is only that the threshold must exceed
    the attacker count; the round engine defaults it to min(K, num_attackers +
    1)).  base — "fedavg" (default: the fused kernel), "median" or
    "trimmed_mean", configured by base_cfg.  server_lr — a finite float > 0,
    default 1.0.

    The global model g the clients started from is the call's center
    (CenteredDefense).

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
        self.server_lr = real_in(defense_config, "server_lr", DEFAULT_SERVER_LR, 0.0, float32=True)
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

    def _rule(self, src, num_examples: List[int], g: torch.Tensor) -> torch.Tensor:
        """src: the client matrix, or one rank's coordinate slice of it."""
        X = src.X
        theta = self.resolve_threshold(X.shape[0])
        if self._base is None:
            out, votes, flipped = ops.rlr_fedavg(X, list(num_examples), g, theta, self.server_lr, diagnostics=True)
        else:
            base = self._base.aggregate_flat if isinstance(src, ClientMatrix) else self._base.aggregate_sharded
            agg = base(src, num_examples)
            votes = ops.sign_vote(X, g)
            out, flipped = ops.rlr_apply(agg, g, votes, theta, self.server_lr, out=agg, count=True)
        self._theta, self._votes, self._flipped = theta, votes, flipped
        return out

    def aggregate_sharded(self, cs, num_examples: List[int],
                          global_flat: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One rank's coordinate range [cs.begin, cs.end): global_flat is the
        center's slice of that range; set_center's vector is the whole model."""
        return self._aggregate(cs, num_examples, global_flat, cs.begin, cs.P)

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
