"""Divide-and-conquer, DnC (Shejwalkar, Houmansadr, "Manipulating the
Byzantine: Optimizing Model Poisoning Attacks and Defenses for Federated
Learning", NDSS 2021, Algorithm 2).

niters times: subsample b coordinates, center them over the clients, score
every client by its squared projection on the top right singular vector of the
centered K x b matrix and drop the ceil(c * f) highest scores; the aggregate is
the mean of the clients every iteration kept.  Colluders that move together
along one direction inside the benign spread (ALIE, Min-Max, Min-Sum of
flr.attacks — the last two from the same paper) dominate that direction's
variance, which neither distances (Krum, Bulyan) nor per-coordinate order (the
trimmed mean, the median) see.  The client rows are model weights; centering
makes the rule independent of the global model.  The reference repository has no
DnC; tests/dnc_ref.py restates the arithmetic of include/flr.h.

Engine: one flr_dnc_select call — per iteration the column gather, the
centering, the fp64 Gram matrix and the one-workgroup spectral kernel — then
flr_rows_mean_keep, which counts the kept rows on the device: nothing comes back
to the host between the selection and the mean.  The kept set and the
diagnostics stay on the device until they are asked for.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional

import torch

from .. import ops
from ..matrix import ClientMatrix
from ._config import int_in, real_in
from .base_defense import BaseDefense, Updates

DEFAULT_FILTER_FRAC = 1.0
DEFAULT_NITERS = 1
DEFAULT_SUBSAMPLE_DIM = 10000
DEFAULT_POWER_ITERS = 32
MAX_CLIENTS = 1024       # flr_dnc_select: one lane per client in the spectral workgroup
MAX_SUBSAMPLE_DIM = 65536


class DnCDefense(BaseDefense):
    """Config: num_malicious — f, an int >= 0; filter_frac — c (default 1.0):
    every iteration removes nremove = min(K - 1, ceil(c * f)) clients; niters
    (default 1, at most 16); subsample_dim — b (default 10000, at most 65536),
    used as min(b, P); power_iters (default 32, at most 1024); seed (default 0):
    call n of an object samples with seed + n, so successive rounds see
    different coordinates and a rerun reproduces them.

    When no client survives every iteration the first iteration's set is used
    (get_metrics()["fallback"]).  A client with a NaN or an inf among the sampled
    coordinates is never kept; if every client is such a row the aggregate is
    NaN in every coordinate.

    num_examples is ignored: the rule is unweighted, as Krum's."""

    # whole rows (the K x K Gram matrix): the engine takes the all-gather exchange
    supports_sharded = False
    # the sampled columns are positions: not invariant under a coordinate permutation
    order_free = False

    def __init__(self, defense_config: Dict[str, Any]):
        super().__init__(defense_config)
        cfg = defense_config
        self.num_malicious = int_in(cfg, "num_malicious", 0, 0)
        self.filter_frac = real_in(cfg, "filter_frac", DEFAULT_FILTER_FRAC, 0.0, closed=True)
        self.niters = int_in(cfg, "niters", DEFAULT_NITERS, 1, ops.DNC_MAX_ITERS)
        self.subsample_dim = int_in(cfg, "subsample_dim", DEFAULT_SUBSAMPLE_DIM, 1, MAX_SUBSAMPLE_DIM)
        self.power_iters = int_in(cfg, "power_iters", DEFAULT_POWER_ITERS, 1, ops.DNC_MAX_POWER_ITERS)
        self.seed = int_in(cfg, "seed", 0, -(1 << 63), (1 << 64) - 1)
        self.calls = 0
        self.nremove = 0
        # device results of the last call
        self._keep = self._count = self._scores = self._cols = self._flags = None
        self._published = True
        self._selected: List[int] = []
        self._rejected: List[int] = []
        self._client_scores: List[float] = []

    def _nremove(self, K: int) -> int:
        """The clients removed per iteration; raises before any device work."""
        if K < 1:
            raise ValueError("DnC needs at least one client")
        if K > MAX_CLIENTS:
            raise ValueError(f"DnC handles at most {MAX_CLIENTS} clients, got {K}")
        return min(K - 1, math.ceil(self.filter_frac * self.num_malicious))

    def aggregate_flat(self, cm: ClientMatrix, num_examples: List[int]) -> torch.Tensor:
        self.nremove = self._nremove(cm.K)
        seed = self.seed + self.calls
        self.calls += 1
        self._keep, self._count, self._scores, self._cols, self._flags = ops.dnc_select(
            cm.X, min(self.subsample_dim, cm.P), self.niters, self.nremove, self.power_iters, seed=seed,
            diagnostics=True)
        self._published = False
        return ops.rows_mean_keep(cm.X, self._keep)

    def _check_clients(self, K: int) -> None:
        self._nremove(K)

    def _publish(self) -> None:
        """The kept set and the last iteration's scores, fetched once per call."""
        if self._published:
            return
        keep = self._keep.cpu().tolist()
        self._selected = [i for i, k in enumerate(keep) if k]
        self._rejected = [i for i, k in enumerate(keep) if not k]
        self._client_scores = self._scores[-1].cpu().tolist()
        self._published = True

    @property
    def selected_clients(self) -> List[int]:
        self._publish()
        return self._selected

    @property
    def rejected_clients(self) -> List[int]:
        self._publish()
        return self._rejected

    @property
    def client_scores(self) -> List[float]:
        self._publish()
        return self._client_scores

    def sampled_columns(self) -> Optional[torch.Tensor]:
        """The last call's columns, int64 [niters, b] on the device (None before a call)."""
        return self._cols

    def detect_malicious(self, client_updates: Updates = None, num_examples: List[int] = None) -> List[int]:
        """The rows the last call rejected."""
        return list(self.rejected_clients)

    def get_metrics(self) -> Dict[str, Any]:
        m = {"defense_type": "dnc", "num_malicious": self.num_malicious, "filter_frac": self.filter_frac,
             "niters": self.niters, "subsample_dim": self.subsample_dim, "power_iters": self.power_iters,
             "seed": self.seed, "calls": self.calls, "nremove": self.nremove, "kept_count": None,
             "fallback": False, "scores": []}
        if self._keep is not None:
            m["kept_count"] = int(self._count.item())
            m["fallback"] = bool(int(self._flags.item()) & 1)
            m["scores"] = self._scores.cpu().tolist()
        return m

    def __repr__(self) -> str:
        return (f"DnCDefense(f={self.num_malicious}, c={self.filter_frac}, niters={self.niters}, "
                f"b={self.subsample_dim})")
