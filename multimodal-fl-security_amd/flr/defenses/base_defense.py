"""Defense plugin interface (mirror of src/defenses/base_defense.py:13-97).

``aggregate(client_updates, num_examples) -> List[Tensor]`` keeps the
reference signature.  ``client_updates`` may be the reference's
``List[List[Tensor]]`` (any device; converted to a device client matrix) or a
:class:`flr.matrix.ClientMatrix` (zero-copy, the engine's own round path).
Results are returned on the device the updates came from.
"""
from __future__ import annotations

from abc import ABC, abstractmethod
from typing import Any, Dict, List, Optional, Sequence, Union

import torch

from .. import ops
from ..matrix import ClientMatrix

Updates = Union[ClientMatrix, Sequence[Sequence[torch.Tensor]]]


def as_matrix(client_updates: Updates) -> ClientMatrix:
    if isinstance(client_updates, ClientMatrix):
        return client_updates
    return ClientMatrix.from_updates(client_updates)


def source_device(client_updates: Updates) -> torch.device:
    if isinstance(client_updates, ClientMatrix):
        return client_updates.device
    return client_updates[0][0].device


class BaseDefense(ABC):
    """Abstract defense (base_defense.py:13-71).

    Subclasses implement ``aggregate_flat(cm, num_examples) -> [P] tensor``
    on a device client matrix; ``aggregate`` adapts the reference signature.
    """

    def __init__(self, defense_config: Dict[str, Any]):
        self.config = defense_config
        self.name = self.__class__.__name__

    @abstractmethod
    def aggregate_flat(self, cm: ClientMatrix, num_examples: List[int]) -> torch.Tensor:
        ...

    def _check_clients(self, K: int) -> None:
        """A defense's size rules for K clients (raises ValueError); the default has none."""

    def _matrix(self, client_updates: Updates) -> ClientMatrix:
        # the size rules first: a list input is not even copied to the device
        self._check_clients(client_updates.K if isinstance(client_updates, ClientMatrix) else len(client_updates))
        return as_matrix(client_updates)

    def aggregate(self, client_updates: Updates, num_examples: List[int]) -> List[torch.Tensor]:
        cm = self._matrix(client_updates)
        flat = self.aggregate_flat(cm, num_examples)
        return cm.unflatten(flat, source_device(client_updates))

    # aggregate_flat (and aggregate_sharded, where there is one) takes the
    # round's global model as global_flat=: the round engine passes it, and runs
    # the round in torch order, where that vector lines up with the columns
    takes_global = False

    # Coordinate-sharded form (flr.shard): aggregate one GPU's coordinate
    # range of all K clients; returns the [cs.n] slice of the aggregate.
    # Defenses that need whole rows (norms, dots) do not implement it and run
    # on the all-gathered matrix instead.
    supports_sharded = False
    # The aggregate's coordinate i depends only on column i and on row-level
    # quantities invariant under one common permutation of the coordinates
    # (pairwise distances, row selections): the round engine may then hand
    # over the client matrix in the trainer's own coordinate order (tap-major
    # conv weights) and permute only the aggregated vector back.
    order_free = False

    def aggregate_sharded(self, cs, num_examples: List[int]) -> torch.Tensor:
        raise NotImplementedError(f"{self.name} has no coordinate-sharded form")

    def detect_malicious(self, client_updates: Updates, num_examples: List[int]) -> List[int]:
        return []

    def get_metrics(self) -> Dict[str, Any]:
        return {}

    def __repr__(self) -> str:
        return f"{self.name}(config={self.config})"


def _flat(params: Union[torch.Tensor, Sequence[torch.Tensor]]) -> torch.Tensor:
    """A vector or a parameter list as one detached flat float32 vector."""
    if isinstance(params, torch.Tensor):
        return params.detach().reshape(-1).float()
    return torch.cat([p.detach().reshape(-1).float() for p in params])


class CenteredDefense(BaseDefense):
    """Base of the defenses that start from the global model the clients
    trained from.  A subclass implements ``_rule(src, num_examples, center) ->
    [n] tensor`` on a ClientMatrix (or, with supports_sharded, a CoordSlice).

    The center of a call, in this order: global_flat when given (the round
    engine's path: the round's global model); the vector of set_center(), used
    by the next call only; this object's own previous result when it has the
    same length (the reference's loop, which passes only the updates: the
    previous result is the global model the clients started from); on a first
    call the coordinate-wise lower median of the rows."""

    takes_global = True

    def __init__(self, defense_config: Dict[str, Any]):
        super().__init__(defense_config)
        self._center: Optional[torch.Tensor] = None    # set_center's vector, for the next call
        self._previous: Optional[torch.Tensor] = None  # the last result (a tensor of this object's own)

    def set_center(self, center: Union[torch.Tensor, Sequence[torch.Tensor], None]) -> None:
        """The global model of the next aggregate call (a flat vector or a
        parameter list, e.g. the initial global model); None withdraws it.  The
        calls after that continue from their own previous result."""
        self._center = None if center is None else _flat(center)

    def _resolve_center(self, X: torch.Tensor, given: Optional[torch.Tensor] = None, begin: int = 0,
                        P: Optional[int] = None) -> torch.Tensor:
        """The float32 contiguous center of X's n columns on X's device.  X
        covers the coordinates [begin, begin + n) of P (default: all of them):
        `given` is the center of that range, set_center's vector the whole
        model.  set_center's vector is spent once a center is resolved, not when
        this raises."""
        n = X.shape[1]
        if given is None and self._center is not None:
            P = n if P is None else P
            if self._center.numel() != P:
                raise ValueError(f"the center holds {self._center.numel()} coordinates, the updates {P}")
            given = self._center[begin:begin + n]
        if given is not None:
            if given.numel() != n:
                raise ValueError(f"the center holds {given.numel()} coordinates, the updates {n}")
            center = given.detach().reshape(-1).to(device=X.device, dtype=torch.float32).contiguous()
        elif self._previous is not None and self._previous.numel() == n and self._previous.device == X.device:
            center = self._previous
        else:
            center = ops.median_lower(X)
        self._center = None
        return center

    @abstractmethod
    def _rule(self, src, num_examples: List[int], center: torch.Tensor) -> torch.Tensor:
        ...

    def _aggregate(self, src, num_examples: List[int], given: Optional[torch.Tensor], begin: int = 0,
                   P: Optional[int] = None) -> torch.Tensor:
        center = self._resolve_center(src.X, given, begin, P)
        self._previous = out = self._rule(src, num_examples, center)
        return out

    def aggregate_flat(self, cm: ClientMatrix, num_examples: List[int],
                       global_flat: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self._aggregate(cm, num_examples, global_flat)

    def aggregate(self, client_updates: Updates, num_examples: List[int],
                  global_params: Optional[List[torch.Tensor]] = None) -> List[torch.Tensor]:
        cm = self._matrix(client_updates)
        flat = self.aggregate_flat(cm, num_examples, None if global_params is None else _flat(global_params))
        # a copy: the caller may update the returned parameters in place, and
        # the next call starts from this result
        return cm.unflatten(flat.clone(), source_device(client_updates))


class NoDefense(BaseDefense):
    """FedAvg: sum(n_i * u_i) / sum(n_i) (base_defense.py:80-97) on the flr_fedavg kernel."""

    def __init__(self, defense_config: Dict[str, Any] = None):
        super().__init__(defense_config or {})

    def aggregate_flat(self, cm: ClientMatrix, num_examples: List[int]) -> torch.Tensor:
        return ops.fedavg(cm.X, list(num_examples))

    supports_sharded = True
    order_free = True

    def aggregate_sharded(self, cs, num_examples: List[int]) -> torch.Tensor:
        return ops.fedavg(cs.X, list(num_examples))
