"""Bulyan (El Mhamdi, Guerraoui, Rouault, "The Hidden Vulnerability of
Distributed Learning in Byzantium", ICML 2018).

n clients, f = num_malicious, theta = n - 2f, beta = theta - 2f; n >= 4f + 3.
Stage 1 re-runs Krum on the shrinking set: theta times, score the clients
still alive against each other and move the best one to the selection
(flr_krum_select_iter: on the device, no host round trip between the picks).
Stage 2 is coordinate-wise over the theta selected rows: the mean of the beta
values closest to the lower median (flr_median_window_mean_rows, no gather
copy of the selection).  Pipeline as KrumDefense: flr_pairwise_l2 -> selection
-> one pass over the selected rows.  The reference repository has no Bulyan;
tests/bulyan_ref.py restates the two stages from the oracle's Krum scores.
"""
from __future__ import annotations

from typing import Any, Dict

import torch

from .. import ops
from .base_defense import BaseDefense
from .krum import KrumDefense

MAX_ROWS = 128  # rows the window-mean kernel sorts in one lane's registers (include/flr.h)


class BulyanDefense(KrumDefense):
    """Config: num_malicious, pairwise_method (multi_k is ignored: the
    selection holds theta = n - 2f clients).  selected_clients: the theta
    picks in pick order; rejected_clients: the rest, ascending;
    client_scores: the first iteration's Krum scores."""

    def __init__(self, defense_config: Dict[str, Any]):
        super().__init__(defense_config)
        self.theta = 0
        self.beta = 0

    # the window mean reads the selected rows whole: no dead-tap deferral
    supports_dead_rows = False

    def _sizes(self, n: int) -> None:
        """theta and beta for n clients; raises before any device work."""
        f = self.num_malicious
        if n < 4 * f + 3:
            raise ValueError(
                f"Bulyan requires n >= 4f + 3. Got n={n}, f={f}. Need at least {4 * f + 3} clients.")
        theta = n - 2 * f
        if theta > MAX_ROWS:
            raise ValueError(f"Bulyan's median-window mean sorts at most {MAX_ROWS} selected rows "
                             f"(the 128-row limit). Got theta = n - 2f = {theta} (n={n}, f={f}).")
        self.theta, self.beta = theta, theta - 2 * f

    def _pick(self) -> torch.Tensor:
        """The iterated selection on self.distances; returns the int32 picks."""
        self.scores_device, self.order_device = ops.krum_select_iter(self.distances, self.num_malicious, self.theta)
        return self.order_device

    def _combine(self, src, picked: torch.Tensor) -> torch.Tensor:
        """The window mean of src's columns (a rank's coordinate range, or all)."""
        return ops.median_window_mean(src.X, self.beta, rows=picked[: self.theta])

    def publish(self) -> None:
        picked = self.order_device.cpu().tolist()
        self.client_scores = self.scores_device.cpu().tolist()
        self.selected_clients = picked[: self.theta]
        self.rejected_clients = picked[self.theta:]

    _check_clients = _sizes  # for aggregate(): before a list input is copied to the device
    aggregate = BaseDefense.aggregate  # multi_k is ignored: no single-Krum shortcut

    def get_metrics(self) -> Dict[str, Any]:
        m = super().get_metrics()
        m.update({"defense_type": "bulyan", "theta": self.theta, "beta": self.beta})
        return m

    def __repr__(self) -> str:
        return f"BulyanDefense(f={self.num_malicious})"
