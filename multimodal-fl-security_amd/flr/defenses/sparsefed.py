"""SparseFed (Panda, Mahloujifar, Bhagoji, Chakraborty, Mittal, "SparseFed:
Mitigating Model Poisoning Attacks in Federated Learning with Sparsification",
AISTATS 2022, Algorithm 1).

With u_i = x_i - g the update of client i from the global model g, W a
server-side error memory that lives across the rounds, and rho a momentum:

  u_i *= min(1, L / ||u_i||);   a = (1 / n) * sum of the n clipped u_i
  U = rho * U + a               (rho = 0: no U)
  W = W + U
  g' = g + W on the k coordinates where |W| is largest; there W = U = 0
  g' = g elsewhere; those coordinates stay in W for later rounds

The attacker's reach is bounded by the clipping and by having to win the top-k
against the honest majority's accumulated direction; the rule needs no attacker
count and no server data.  It is the one rule here that keeps state in parameter
space (FoolsGold keeps it in client space).  The client rows are model weights.
The reference repository has no SparseFed; tests/sparsefed_ref.py restates the
arithmetic of include/flr.h.

Engine: flr_row_norms, flr_sparsefed_weights (one workgroup),
flr_sparsefed_accumulate (the one pass over the client matrix, which also
counts the first digit of the select), flr_topk_abs_select (an exact radix
select on the device) and flr_sparsefed_apply, enqueued back to back with no
host round trip; the diagnostics stay on the device until they are asked for.

The round engine's checkpoint does not carry W (or U): a resumed run starts from
an empty memory.
"""
from __future__ import annotations

import math
import numbers
import struct
from typing import Any, Dict, List, Optional, Union

import torch

from .. import ops
from ..matrix import ClientMatrix
from ._config import real_in
from .base_defense import CenteredDefense, Updates

DEFAULT_K = 0.05  # this project's choice: the paper tunes k per task
MAX_CLIENTS = ops.SPARSEFED_MAX_CLIENTS


class SparseFedDefense(CenteredDefense):
    """Config: k — an int in [1, P] (checked against P at the call), or a
    float in (0, 1] meaning ceil(k * P); the default, 0.05, is this project's
    choice (the paper tunes k per task).  clip_norm — a finite float > 0, or
    "median" (default): the lower median of the clients' finite update norms,
    this project's adaptive choice as FLAME's bound is (the paper's L is a tuned
    constant).  momentum — rho, a float in [0, 1), default 0.0.

    The global model g the updates are taken from is the call's center
    (CenteredDefense).

    State: W, and U when momentum != 0, float32 [P] on the device (P * 4 bytes
    each: 47 MB at P = 11.8 M), from the first call on.  reset() drops it; a call
    with another P or device raises.  The round engine's checkpoint does not
    carry it.

    A client with a NaN or an inf gets weight 0 (get_metrics()["bad_rows"]) and
    its row is not read.  A coordinate whose memory overflows is set to 0
    (get_metrics()["dropped"]).

    num_examples is ignored: the rule brings its own weights."""

    # whole rows (the norms) and a selection over all P coordinates: the engine takes the all-gather exchange
    supports_sharded = False
    # the center is a vector in torch order: the round runs in torch order
    order_free = False

    def __init__(self, defense_config: Dict[str, Any]):
        super().__init__(defense_config)
        cfg = defense_config
        k = cfg.get("k", DEFAULT_K)
        bad = f"k must be an integer >= 1 or a float in (0, 1], got {k!r}"
        if isinstance(k, bool) or not isinstance(k, numbers.Real) or math.isnan(k):
            raise ValueError(bad)
        if isinstance(k, numbers.Integral):
            if k < 1:
                raise ValueError(bad)
            self.k: Union[int, float] = int(k)
        else:
            if not 0.0 < k <= 1.0:
                raise ValueError(bad)
            self.k = float(k)
        clip = cfg.get("clip_norm", "median")
        if isinstance(clip, str):
            if clip != "median":
                raise ValueError(f"clip_norm must be 'median' or a finite number > 0, got {clip!r}")
            self.clip_norm: Union[str, float] = clip
        else:
            self.clip_norm = real_in(cfg, "clip_norm", 0.0, 0.0, or_else=" or 'median'")
        self.momentum = real_in(cfg, "momentum", 0.0, 0.0, closed=True, float32=True)
        if not self.momentum < 1.0 or not float(torch.tensor(self.momentum, dtype=torch.float32)) < 1.0:
            raise ValueError(f"momentum must be in [0, 1) (in float32), got {self.momentum!r}")
        self._W: Optional[torch.Tensor] = None
        self._U: Optional[torch.Tensor] = None
        self._k: Optional[int] = None  # the count the last call resolved
        self._sel = self._stats = self._flags = self._dropped = self._mask = None  # device results of the last call

    def resolve_k(self, P: int) -> int:
        """The number of coordinates applied among P."""
        if isinstance(self.k, int):
            if self.k > P:
                raise ValueError(f"k {self.k} exceeds the {P} coordinates of this call")
            return self.k
        return min(P, max(1, math.ceil(self.k * P)))

    def _check_clients(self, K: int) -> None:
        """Raises before any device work."""
        if K < 1:
            raise ValueError("SparseFed needs at least one client")
        if K > MAX_CLIENTS:
            raise ValueError(f"SparseFed handles at most {MAX_CLIENTS} clients, got {K}")

    def reset(self) -> None:
        """Drops the memory (W and U return to the allocator): the next call
        starts from zero, at any P."""
        self._W = self._U = None

    def memory(self) -> Optional[torch.Tensor]:
        """W, float32 [P] on the device (None before a call)."""
        return self._W

    def momentum_memory(self) -> Optional[torch.Tensor]:
        """U, float32 [P] on the device (None with momentum == 0 or before a call)."""
        return self._U

    def mask(self) -> Optional[torch.Tensor]:
        """The last call's selection: a device uint8 [P] tensor (None before a call)."""
        return self._mask

    def aggregate_flat(self, cm: ClientMatrix, num_examples: List[int],
                       global_flat: Optional[torch.Tensor] = None) -> torch.Tensor:
        # the size rules before the center is resolved: set_center's vector outlives a refused call
        self._check_clients(cm.K)
        self.resolve_k(cm.P)
        if self._W is not None and (self._W.numel() != cm.P or self._W.device != cm.device):
            raise ValueError(f"the memory holds {self._W.numel()} coordinates on {self._W.device}, this call "
                             f"{cm.P} on {cm.device}: reset() starts a new one")
        return super().aggregate_flat(cm, num_examples, global_flat)

    def _rule(self, cm: ClientMatrix, num_examples: List[int], g: torch.Tensor) -> torch.Tensor:
        k = self.resolve_k(cm.P)
        if self._W is None:
            self._W = torch.zeros(cm.P, dtype=torch.float32, device=cm.device)
            self._U = torch.zeros_like(self._W) if self.momentum != 0.0 else None
        norms = ops.row_norms(cm.X, center=g)
        beta, self._stats, self._flags = ops.sparsefed_weights(
            norms, None if self.clip_norm == "median" else self.clip_norm, diagnostics=True)
        _, hist, self._dropped = ops.sparsefed_accumulate_(cm.X, g, beta, self._W, self._U, self.momentum,
                                                           diagnostics=True)
        self._sel = ops.topk_abs_select(self._W, k, hist=hist)
        out, self._mask = ops.sparsefed_apply_(g, self._W, self._sel, U=self._U, mask=True)
        self._k = k
        return out

    def detect_malicious(self, client_updates: Updates = None, num_examples: List[int] = None) -> List[int]:
        """Always []: the rule judges coordinates, not clients."""
        return []

    def get_metrics(self) -> Dict[str, Any]:
        m = {"defense_type": "sparsefed", "k": self.k if self._k is None else self._k, "clip_norm": self.clip_norm,
             "momentum": self.momentum, "clipped": None, "dropped": None, "threshold": None, "bad_rows": False}
        if self._sel is not None:
            L, _, clipped = self._stats.cpu().tolist()
            m["clip_norm"] = L
            m["clipped"] = int(clipped)
            m["dropped"] = int(self._dropped.item())
            m["threshold"] = struct.unpack("<f", struct.pack("<I", int(self._sel[0].item()) & 0xffffffff))[0]
            m["bad_rows"] = bool(int(self._flags.item()) & 2)
        return m

    def __repr__(self) -> str:
        return f"SparseFedDefense(k={self.k}, clip_norm={self.clip_norm!r}, momentum={self.momentum})"
