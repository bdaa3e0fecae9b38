"""FoolsGold (Fung, Yoon, Beschastnikh, "The Limitations of Federated Learning
in Sybil Settings", RAID 2020, Algorithm 1).

Sybils work towards one goal, so their updates resemble each other more than
honest clients' do.  With u_i = x_i - g the update of client i from the global
model g, and H_i the running sum of its updates over the rounds:

  cs_ij = cos(H_i, H_j);  v_i = max_j cs_ij
  pardoning: cs_ij *= v_i / v_j when v_i < v_j  (an honest client that happens
             to resemble a sybil is not punished with it)
  w_i = 1 - max_j cs_ij, rescaled by the largest, through the logit with
        confidence kappa, clipped to [0, 1]: alpha_i
  g' = g + sum_i (alpha_i / sum alpha) * u_i

The rule needs no attacker count and no server data: the defense for the
attackers that act in concert (the colluding attacks' identical rows, a common
backdoor), which every attack of flr.attacks does.  The client rows are model
weights; clients are positional (row i is client i in every call).  The
reference repository has no FoolsGold; tests/foolsgold_ref.py restates the
arithmetic of include/flr.h.

Engine: flr_rows_accumulate (the history), flr_rows_gram (the K x K Gram matrix
over all P coordinates on the fp64 matrix cores, exact products),
flr_foolsgold_weights (one workgroup) and flr_rows_combine_from, enqueued back
to back with no host round trip; the diagnostics stay on the device until they
are asked for.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import torch

from .. import ops
from ..matrix import ClientMatrix, padded_ld
from ._config import real_in
from .base_defense import CenteredDefense, Updates

DEFAULT_CONFIDENCE = 1.0
MAX_CLIENTS = ops.FOOLSGOLD_MAX_CLIENTS  # one lane per client in the weights workgroup


class FoolsGoldDefense(CenteredDefense):
    """Config: confidence — kappa, a finite float > 0 (default 1.0, the
    paper's); use_memory — bool (default True): the similarity is taken on the
    per-client running sum of updates, a K x P float32 matrix kept on the
    device from the first call on (K * P * 4 bytes: 6 GB at K = 128, P = 11.8 M)
    and one more pass over the client matrix per call; False: on this call's
    updates alone, no history is allocated.

    The global model g the updates are taken from is the call's center
    (CenteredDefense).

    When every weight is 0 (all clients alike, or every row non-finite) the
    result is the center: no update (get_metrics()["no_update"]).  A client
    with a NaN or an inf gets weight 0 (get_metrics()["bad_rows"]) and its row
    is not read by the combination; with use_memory its history stays
    non-finite, so it is rejected until reset().

    num_examples is ignored: the rule brings its own weights."""

    # whole rows (the K x K Gram matrix): the engine takes the all-gather exchange
    supports_sharded = False
    # the center is a vector in torch order: the round runs in torch order
    order_free = False

    def __init__(self, defense_config: Dict[str, Any]):
        super().__init__(defense_config)
        self.confidence = real_in(defense_config, "confidence", DEFAULT_CONFIDENCE, 0.0)
        m = defense_config.get("use_memory", True)
        if not isinstance(m, bool):
            raise ValueError(f"use_memory must be a bool, got {m!r}")
        self.use_memory = m
        self.calls = 0
        self._history: Optional[torch.Tensor] = None   # H, float32 [K, P]
        self._alpha = self._beta = self._maxcos = self._flags = None  # device results of the last call

    @staticmethod
    def _check_size(K: int) -> None:
        """Raises before any device work."""
        if K < 1:
            raise ValueError("FoolsGold needs at least one client")
        if K > MAX_CLIENTS:
            raise ValueError(f"FoolsGold handles at most {MAX_CLIENTS} clients, got {K}")

    def _check_clients(self, K: int) -> None:
        self._check_size(K)

    def reset(self) -> None:
        """Drops the history (its memory returns to the allocator): the next
        call starts a new one, of any shape."""
        self._history = None

    def history(self) -> Optional[torch.Tensor]:
        """H, float32 [K, P] on the device (None without memory or before a call)."""
        return self._history

    def aggregate_flat(self, cm: ClientMatrix, num_examples: List[int],
                       global_flat: Optional[torch.Tensor] = None) -> torch.Tensor:
        # the size rules before the center is resolved: set_center's vector outlives a refused call
        self._check_size(cm.K)
        if self._history is not None and tuple(self._history.shape) != (cm.K, cm.P):
            raise ValueError(f"the history holds {self._history.shape[0]} clients x {self._history.shape[1]} "
                             f"coordinates, this call {cm.K} x {cm.P}: reset() starts a new one")
        return super().aggregate_flat(cm, num_examples, global_flat)

    def _rule(self, cm: ClientMatrix, num_examples: List[int], g: torch.Tensor) -> torch.Tensor:
        if self.use_memory:
            if self._history is None or self._history.device != cm.device:
                # the client matrix's padded row stride: the kernels' 16-byte loads
                self._history = torch.zeros((cm.K, padded_ld(cm.P)), dtype=torch.float32,
                                            device=cm.device)[:, :cm.P]
            ops.rows_accumulate_(self._history, cm.X, g)
            G = ops.rows_gram(self._history)
        else:
            G = ops.rows_gram(cm.X, center=g)
        self._alpha, self._beta, self._maxcos, self._flags = ops.foolsgold_weights(G, self.confidence,
                                                                                   diagnostics=True)
        out = ops.rows_combine_from(cm.X, g, self._beta)
        self.calls += 1
        return out

    @property
    def client_weights(self) -> List[float]:
        """alpha of the last call, one per client ([] before a call)."""
        return [] if self._alpha is None else self._alpha.cpu().tolist()

    def detect_malicious(self, client_updates: Updates = None, num_examples: List[int] = None) -> List[int]:
        """The rows with alpha == 0 in the last call."""
        if self._alpha is None:
            return []
        return torch.nonzero(self._alpha == 0).reshape(-1).cpu().tolist()

    def get_metrics(self) -> Dict[str, Any]:
        m = {"defense_type": "foolsgold", "confidence": self.confidence, "use_memory": self.use_memory,
             "calls": self.calls, "weights": [], "max_cosine": [], "no_update": False, "bad_rows": False}
        if self._alpha is not None:
            flags = int(self._flags.item())
            m["weights"] = self._alpha.cpu().tolist()
            m["max_cosine"] = self._maxcos.cpu().tolist()
            m["no_update"] = bool(flags & 1)
            m["bad_rows"] = bool(flags & 2)
        return m

    def __repr__(self) -> str:
        return f"FoolsGoldDefense(confidence={self.confidence}, use_memory={self.use_memory})"
