"""FLAME (Nguyen et al., "FLAME: Taming Backdoors in Federated Learning",
USENIX Security 2022, Algorithm 1).

A backdoored update points elsewhere than the honest ones and, boosted to
survive the average (model replacement), is longer.  With u_i = x_i - g the
update of client i from the global model g:

  d_ij = 1 - cos(u_i, u_j)
  clustering: HDBSCAN(min_cluster_size = K // 2 + 1, min_samples = 1,
              allow_single_cluster = True) on d; the cluster is admitted
  S = the median of ||u_i|| over all clients;  u_i *= min(1, S / ||u_i||)
  g' = g + (1 / L) * sum of the L admitted, clipped u_i + N(0, (lambda * S)^2)

With min_samples = 1 the mutual reachability distance is d itself, and with a
majority min_cluster_size the condensed tree cannot split: the cluster is the
first single-linkage component that reaches min_cluster_size points
(include/flr.h states both facts; tests/test_flame_host.py checks the closed form
against sklearn's HDBSCAN).  Because the cluster is cut the moment it reaches
that size, FLAME admits about half the clients — min_cluster_size or one more —
however few attack: that is the published rule; min_cluster_size is the knob.

The rule needs no attacker count and no server data.  The client rows are model
weights.  The reference repository has no FLAME; tests/flame_ref.py restates the
arithmetic of include/flr.h.

Engine: flr_rows_gram (the K x K Gram matrix over all P coordinates on the fp64
matrix cores, exact products), flr_flame_select (one workgroup: distances,
clustering, median, weights, sigma), flr_rows_combine_from and flr_add_gaussian
(Philox4x32-10, Box-Muller), enqueued back to back with no host round trip; the
diagnostics stay on the device until they are asked for.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import torch

from .. import ops
from ..matrix import ClientMatrix
from ._config import int_in, real_in
from .base_defense import CenteredDefense, Updates

DEFAULT_NOISE_LAMBDA = 0.001  # the paper's value for image and text models
MAX_CLIENTS = ops.FLAME_MAX_CLIENTS  # one lane per client in the selection workgroup


class FlameDefense(CenteredDefense):
    """Config: noise_lambda — lambda, a finite float >= 0 (default 0.001, the
    paper's for image and text models; 0: no noise kernel is launched);
    min_cluster_size — None (default: K // 2 + 1, the paper's) or an int m with
    2 m > K and m <= K, checked per call; on — "updates" (default: the cosines of
    x_i - g) or "weights" (the paper's Algorithm 1 read literally: the cosines
    of the models x_i; the norms that are clipped stay those of the updates);
    seed — an int (default 0): call n of an object draws its noise with
    draw_stream = n, so successive rounds see different noise and a rerun
    reproduces it.

    The global model g the updates are taken from is the call's center
    (CenteredDefense).

    With fewer than min_cluster_size clients with finite rows there is no
    cluster and the result is the center: no update
    (get_metrics()["no_update"]).  A client with a NaN or an inf is rejected
    (get_metrics()["bad_rows"]) and its row is not read by the combination.

    num_examples is ignored: the rule brings its own weights."""

    # whole rows (the K x K Gram matrix): the engine takes the all-gather exchange
    supports_sharded = False
    # the center is a vector in torch order: the round runs in torch order
    order_free = False

    def __init__(self, defense_config: Dict[str, Any]):
        super().__init__(defense_config)
        cfg = defense_config
        self.noise_lambda = real_in(cfg, "noise_lambda", DEFAULT_NOISE_LAMBDA, 0.0, closed=True)
        m = cfg.get("min_cluster_size")
        if m is not None:
            m = int_in(cfg, "min_cluster_size", 1, 1, MAX_CLIENTS)
        self.min_cluster_size = m
        on = cfg.get("on", "updates")
        if on not in ("updates", "weights"):
            raise ValueError(f"on must be 'updates' or 'weights', got {on!r}")
        self.on = on
        self.seed = int_in(cfg, "seed", 0, -(1 << 63), (1 << 64) - 1)
        self.calls = 0
        self._keep = self._beta = self._sigma = self._stats = self._flags = None  # device results of the last call

    def _check_clients(self, K: int) -> None:
        """Raises before any device work."""
        if K < 1:
            raise ValueError("FLAME needs at least one client")
        if K > MAX_CLIENTS:
            raise ValueError(f"FLAME handles at most {MAX_CLIENTS} clients, got {K}")
        ops.flame_cluster_size(K, self.min_cluster_size)

    def aggregate_flat(self, cm: ClientMatrix, num_examples: List[int],
                       global_flat: Optional[torch.Tensor] = None) -> torch.Tensor:
        # the size rules before the center is resolved: set_center's vector outlives a refused call
        self._check_clients(cm.K)
        return super().aggregate_flat(cm, num_examples, global_flat)

    def _rule(self, cm: ClientMatrix, num_examples: List[int], g: torch.Tensor) -> torch.Tensor:
        if self.on == "updates":
            G, norms = ops.rows_gram(cm.X, center=g), None
        else:
            G, norms = ops.rows_gram(cm.X), ops.row_norms(cm.X, center=g)
        self._keep, self._beta, self._sigma, self._stats, self._flags = ops.flame_select(
            G, self.min_cluster_size, self.noise_lambda, norms, diagnostics=True)
        out = ops.rows_combine_from(cm.X, g, self._beta)
        if self.noise_lambda > 0.0:
            ops.add_gaussian_(out, self._sigma, seed=self.seed, stream=self.calls % 2 ** 32)
        self.calls += 1
        return out

    @property
    def client_weights(self) -> List[float]:
        """beta of the last call, one per client ([] before a call)."""
        return [] if self._beta is None else self._beta.cpu().tolist()

    def detect_malicious(self, client_updates: Updates = None, num_examples: List[int] = None) -> List[int]:
        """The rows the last call rejected (keep == 0)."""
        if self._keep is None:
            return []
        return torch.nonzero(self._keep == 0).reshape(-1).cpu().tolist()

    def get_metrics(self) -> Dict[str, Any]:
        m = {"defense_type": "flame", "noise_lambda": self.noise_lambda, "min_cluster_size": self.min_cluster_size,
             "on": self.on, "seed": self.seed, "calls": self.calls, "admitted": None, "clip_bound": None,
             "threshold": None, "sigma": None, "no_update": False, "bad_rows": False}
        if self._keep is not None:
            S, t, L = self._stats.cpu().tolist()
            flags = int(self._flags.item())
            m["admitted"] = int(L)
            m["clip_bound"] = S
            m["threshold"] = t
            m["sigma"] = float(self._sigma.item())
            m["no_update"] = bool(flags & 1)
            m["bad_rows"] = bool(flags & 2)
        return m

    def __repr__(self) -> str:
        return (f"FlameDefense(noise_lambda={self.noise_lambda}, min_cluster_size={self.min_cluster_size}, "
                f"on={self.on!r})")
