"""Tensor-level wrappers over the flr C ABI (device tensors in, device tensors out).

Each op validates shapes on the host, allocates outputs / workspace with the
PyTorch caching allocator on the tensor's device, and enqueues the HIP
kernels on torch's current stream.  No op has a fallback: a CPU tensor, a
wrong dtype or a missing library raises.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _capi
from ._capi import ptr as _ptr, stream_of as _stream

CHUNK = 64  # coordinates per pairwise chunk; client matrices pad ldx to this
PW_SLICES = 8  # FLR_PW_SLICES: canonical coordinate slices of the pairwise kernels
REFINE_ROWS = 128  # far-cluster rows the Gram path refines per call (include/flr.h, a9)


def _check_matrix(X: torch.Tensor, name: str = "X") -> Tuple[int, int, int]:
    if not isinstance(X, torch.Tensor) or not X.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA/HIP tensor (the engine has no CPU path)")
    if X.dtype != torch.float32 or X.dim() != 2 or X.stride(1) != 1 or X.stride(0) < X.shape[1]:
        raise ValueError(f"{name} must be a row-major float32 [K, P] matrix (got {X.dtype}, "
                         f"shape {tuple(X.shape)}, strides {X.stride()})")
    return X.shape[0], X.shape[1], X.stride(0)


def _check_vector(t, n: int, device, name: str, dtype=torch.float32) -> None:
    if not isinstance(t, torch.Tensor) or t.device != device or t.dtype != dtype or not t.is_contiguous() \
            or t.numel() != n:
        raise ValueError(f"{name} must be a contiguous {str(dtype).replace('torch.', '')} [{n}] vector on {device}")


def _out_vector(out: Optional[torch.Tensor], n: int, device, dtype=torch.float32,
                name: Optional[str] = "out") -> torch.Tensor:
    """A new output vector, or the caller's, checked (name=None: taken as it
    is, by the ops that never checked theirs)."""
    if out is None:
        return torch.empty(n, dtype=dtype, device=device)
    if name is not None:
        _check_vector(out, n, device, name, dtype)
    return out


def _examples(num_examples, K: int, device) -> torch.Tensor:
    """num_examples as the int64 [K] device vector of the FedAvg kernels."""
    n = torch.as_tensor(num_examples, dtype=torch.int64).to(device).contiguous()
    if n.numel() != K:
        raise ValueError(f"num_examples has {n.numel()} entries for {K} clients")
    return n


def _ws(nbytes: int, device) -> Tuple[torch.Tensor, int]:
    """A workspace of nbytes and its 256-byte aligned address inside it."""
    ws = torch.empty(max(nbytes, 256) + 256, dtype=torch.uint8, device=device)
    return ws, ws.data_ptr() + (-ws.data_ptr()) % 256


def pairwise_l2(X: torch.Tensor, method: str = "gram", events=None, comm=None,
                tap_blocks: Optional[Sequence[Tuple[int, int, int, int]]] = None, dead=None) -> torch.Tensor:
    """K×K float64 distances, D[i][j] = fp32 ||X_i - X_j|| (krum.py:73-99).

    method: "gram" (centred Gram on MFMA), "direct" (exact fp32 differences,
    fp32/fp64 partial sums) or "reference" (the reference's own torch.norm
    accumulation, bit-identical D over the reference's coordinate order:
    X's columns in that order, or tap_blocks [(off, Cout, Cin, KK), ...]
    naming the convolution weights X holds tap-major — a training-order
    matrix, no reordered copy; include/flr.h flr_pairwise_l2_reference_tap).
    events: optional (begin, end) raw hipEvent_t handles recorded around the
    main MFMA kernel (flr.timing.HipEventPair).
    comm: optional flr.shard.Comm for the reference mode: every rank holds the
    whole X, computes 1/world of the pair tiles and one all-reduce (sum, exact:
    one non-zero term per pair) of the 8·K² bytes of D gives every rank D.
    dead: optional (masks, gdead, nneg) with tap_blocks — X's dead-tap slabs
    are not written (FLR_TC_DEFER_DEAD): bit t of masks[b] reads tap t of
    block b from the training-order vector gdead, negated on rows < nneg
    (flr_pairwise_l2_reference_tap_dead; the same D as on the filled X)."""
    K, P, ldx = _check_matrix(X)
    D = torch.empty((K, K), dtype=torch.float64, device=X.device)
    if method == "reference":
        if X.data_ptr() % 16 or ldx % 4:  # the kernels load 16-B pieces of 16-B aligned rows
            if dead is not None:
                raise ValueError("pairwise_l2(dead=): the rows must be 16-B aligned (read in place)")
            Xa = torch.zeros((K, (P + 63) // 64 * 64), dtype=torch.float32, device=X.device)
            Xa[:, :P].copy_(X)
            X, ldx = Xa, Xa.stride(0)
        part, nparts = (0, 1) if comm is None else (comm.rank, comm.world)
        wp, nbytes = _ref_workspace(K, P, X.device, _stream(X))
        taps = [int(v) for blk in (tap_blocks or ()) for v in blk]
        tarr = (ctypes.c_int64 * max(1, len(taps)))(*taps)
        if dead is None:
            _capi.call("flr_pairwise_l2_reference_tap", X.data_ptr(), K, P, ldx, ctypes.addressof(tarr),
                       len(taps) // 4, D.data_ptr(), wp, nbytes, part, nparts, _stream(X))
        else:
            masks, gdead, nneg = dead
            if len(masks) != len(taps) // 4 or gdead.device != X.device or gdead.dtype != torch.float32 \
                    or gdead.numel() < P:
                raise ValueError("pairwise_l2(dead=): one mask per tap block and a float32 P-vector on X's device")
            marr = (ctypes.c_uint64 * max(1, len(masks)))(*[int(m) for m in masks])
            _capi.call("flr_pairwise_l2_reference_tap_dead", X.data_ptr(), K, P, ldx, ctypes.addressof(tarr),
                       len(taps) // 4, ctypes.addressof(marr), gdead.data_ptr(), int(nneg), D.data_ptr(), wp,
                       nbytes, part, nparts, _stream(X))
        if nparts > 1:
            comm.all_reduce_sum(D)
        return D
    if method == "gram":
        ws_fn, fn = "flr_pairwise_l2_workspace", "flr_pairwise_l2"
    elif method == "direct":
        ws_fn, fn = "flr_pairwise_l2_direct_workspace", "flr_pairwise_l2_direct"
    else:
        raise ValueError(f"unknown pairwise method {method!r}")
    nbytes = int(getattr(_capi.lib(), ws_fn)(K, P))
    ws, wp = _ws(nbytes, X.device)
    if events is not None and method == "gram":
        _capi.call("flr_pairwise_l2_ex", X.data_ptr(), K, P, ldx, D.data_ptr(), wp, nbytes, _stream(X), events[0],
                   events[1])
    else:
        _capi.call(fn, X.data_ptr(), K, P, ldx, D.data_ptr(), wp, nbytes, _stream(X))
    return D


def krum_select(D: torch.Tensor, f: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(scores fp64 [K], order int32 [K]) — krum.py:101-131, 149-176."""
    if not D.is_cuda or D.dtype != torch.float64 or D.dim() != 2 or D.shape[0] != D.shape[1]:
        raise ValueError("D must be a square float64 device matrix")
    D = D.contiguous()
    K = D.shape[0]
    scores = torch.empty(K, dtype=torch.float64, device=D.device)
    order = torch.empty(K, dtype=torch.int32, device=D.device)
    _capi.call("flr_krum_select", D.data_ptr(), K, int(f), scores.data_ptr(), order.data_ptr(), _stream(D))
    return scores, order


def krum_select_iter(D: torch.Tensor, f: int, theta: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Bulyan's iterated Krum selection (flr_krum_select_iter): (scores fp64
    [K], the first iteration's Krum scores; picked int32 [K], the theta picks
    in pick order, then the unpicked clients ascending).  All theta iterations
    are enqueued on the current stream: no host synchronisation."""
    if not D.is_cuda or D.dtype != torch.float64 or D.dim() != 2 or D.shape[0] != D.shape[1]:
        raise ValueError("D must be a square float64 device matrix")
    D = D.contiguous()
    K = D.shape[0]
    scores = torch.empty(K, dtype=torch.float64, device=D.device)
    picked = torch.empty(K, dtype=torch.int32, device=D.device)
    nbytes = int(_capi.lib().flr_krum_select_iter_workspace(K))
    ws, wp = _ws(nbytes, D.device)
    _capi.call("flr_krum_select_iter", D.data_ptr(), K, int(f), int(theta), scores.data_ptr(), picked.data_ptr(),
               wp, nbytes, _stream(D))
    return scores, picked


def rows_mean(X: torch.Tensor, rows: torch.Tensor, divisor: Optional[int] = None,
              out: Optional[torch.Tensor] = None, dead=None) -> torch.Tensor:
    """Ordered fp32 sum of X[rows] divided by `divisor` (krum.py:182-192).
    dead: optional (ranges [(off, n), ...], gdead, nneg) — X's dead-tap ranges
    are not written (FLR_DEFER_DEAD=2): row k's value there is gdead's, negated
    for k < nneg (flr_rows_mean_dead; the same bits as over the filled rows)."""
    K, P, ldx = _check_matrix(X)
    rows = rows.to(device=X.device, dtype=torch.int32).contiguous()
    m = rows.numel()
    divisor = m if divisor is None else int(divisor)
    out = _out_vector(out, P, X.device, name=None)
    if dead is None:
        _capi.call("flr_rows_mean", X.data_ptr(), K, P, ldx, rows.data_ptr(), m, divisor, out.data_ptr(),
                   _stream(X))
        return out
    ranges, gdead, nneg = dead
    off = (ctypes.c_int64 * max(1, len(ranges)))(*[int(o) for o, _ in ranges])
    ln = (ctypes.c_int64 * max(1, len(ranges)))(*[int(n) for _, n in ranges])
    _capi.call("flr_rows_mean_dead", X.data_ptr(), K, P, ldx, rows.data_ptr(), m, divisor, ctypes.addressof(off),
               ctypes.addressof(ln), len(ranges), gdead.data_ptr(), int(nneg), out.data_ptr(), _stream(X))
    return out


def fill_dead_ranges(vec: torch.Tensor, ranges, gdead: torch.Tensor, negate: bool) -> torch.Tensor:
    """vec's dead-tap ranges <- gdead's (negated when `negate`): one row of a
    FLR_DEFER_DEAD=2 matrix made whole (flr_copy_rows_neg per range)."""
    st = _stream(vec)
    for o, n in ranges:
        _capi.call("flr_copy_rows_neg", gdead.data_ptr() + 4 * o, n, n, vec.data_ptr() + 4 * o, n, 1,
                   1 if negate else 0, st)
    return vec


def fedavg(X: torch.Tensor, num_examples, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Example-weighted average (base_defense.py:80-97)."""
    K, P, ldx = _check_matrix(X)
    n = _examples(num_examples, K, X.device)
    out = _out_vector(out, P, X.device, name=None)
    _capi.call("flr_fedavg", X.data_ptr(), K, P, ldx, n.data_ptr(), out.data_ptr(), _stream(X))
    return out


def _rows_arg(rows, device):
    return rows.to(device=device, dtype=torch.int32).contiguous()


def trimmed_mean(X: torch.Tensor, t: int, out: Optional[torch.Tensor] = None,
                 rows: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Coordinate-wise mean of sorted ranks [t, m-t) (trimmed_mean.py:74-88)
    over all K rows, or over the row subset `rows` (m = len(rows))."""
    K, P, ldx = _check_matrix(X)
    out = _out_vector(out, P, X.device, name=None)
    if rows is None:
        _capi.call("flr_trimmed_mean", X.data_ptr(), K, P, ldx, int(t), out.data_ptr(), _stream(X))
    else:
        r = _rows_arg(rows, X.device)
        _capi.call("flr_trimmed_mean_rows", X.data_ptr(), K, P, ldx, r.data_ptr(), r.numel(), int(t), out.data_ptr(),
                   _stream(X))
    return out


def median_lower(X: torch.Tensor, out: Optional[torch.Tensor] = None,
                 rows: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Coordinate-wise lower median (trimmed_mean.py:101, 163), optionally of a row subset."""
    K, P, ldx = _check_matrix(X)
    out = _out_vector(out, P, X.device, name=None)
    if rows is None:
        _capi.call("flr_median_lower", X.data_ptr(), K, P, ldx, out.data_ptr(), _stream(X))
    else:
        r = _rows_arg(rows, X.device)
        _capi.call("flr_median_lower_rows", X.data_ptr(), K, P, ldx, r.data_ptr(), r.numel(), out.data_ptr(),
                   _stream(X))
    return out


def median_window_mean(X: torch.Tensor, beta: int, rows: Optional[torch.Tensor] = None,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Bulyan's coordinate-wise rule (flr_median_window_mean_rows): the mean
    of the beta values closest to the lower median, over all K rows or over
    the row subset `rows` (at most 128 rows either way)."""
    K, P, ldx = _check_matrix(X)
    out = _out_vector(out, P, X.device, name=None)
    r = None if rows is None else _rows_arg(rows, X.device)
    m = K if r is None else r.numel()
    _capi.call("flr_median_window_mean_rows", X.data_ptr(), K, P, ldx, _ptr(r), m, int(beta), out.data_ptr(),
               _stream(X))
    return out


COLLUDE_ALIE, COLLUDE_IPM = 0, 1  # FLR_COLLUDE_*


def collude_rows(X: torch.Tensor, nmal: int, mode: int, param: float, mean_out: Optional[torch.Tensor] = None,
                 std_out: Optional[torch.Tensor] = None) -> None:
    """The colluding attacks in place (flr_collude_rows): rows [0, nmal) of X
    <- mu - param * sigma (COLLUDE_ALIE) or -(param * mu) (COLLUDE_IPM), mu and
    sigma the benign rows' [nmal, K) coordinate-wise mean and population
    deviation; mean_out / std_out: optional float32 [P] device vectors that
    receive them."""
    K, P, ldx = _check_matrix(X)
    for name, t in (("mean_out", mean_out), ("std_out", std_out)):
        if t is not None:
            _check_vector(t, P, X.device, name)
    _capi.call("flr_collude_rows", X.data_ptr(), K, P, ldx, int(nmal), int(mode), float(param), _ptr(mean_out),
               _ptr(std_out), _stream(X))


MINMAX_MAX, MINMAX_SUM = 0, 1                    # FLR_MINMAX_*
PERTURB_STD, PERTURB_SIGN, PERTURB_UNIT = 0, 1, 2  # FLR_PERTURB_*


def minmax_rows(X: torch.Tensor, nmal: int, objective: int, perturb: int, global_flat: Optional[torch.Tensor] = None,
                diagnostics: bool = False):
    """The Min-Max / Min-Sum attacks in place (flr_minmax_rows): rows [0, nmal)
    of X <- mu + gamma * p, mu the benign rows' [nmal, K) mean, p = -sigma
    (PERTURB_STD), -sign(mu - g) (PERTURB_SIGN) or -(mu - g) (PERTURB_UNIT, not
    normalised: gamma is relative to this p), g = global_flat, gamma the largest
    strength that keeps the vector within the benign rows' largest mutual
    distance (MINMAX_MAX) or largest distance sum (MINMAX_SUM).  The whole call
    is enqueued on the current stream: no host synchronisation.  Returns gamma
    (float64 device scalar; NaN: a statistic was NaN and no row was written), or
    with diagnostics (gamma, stats float64 [2 * nb + 4] — a_i, b_i, c, R2, S,
    the bound used —, mu float32 [P], sigma float32 [P]) as device tensors."""
    K, P, ldx = _check_matrix(X)
    if global_flat is not None:
        _check_vector(global_flat, P, X.device, "global_flat")
    nmal = int(nmal)
    gamma = torch.empty((), dtype=torch.float64, device=X.device)
    stats = None
    if diagnostics:
        stats = torch.empty(2 * max(K - nmal, 0) + 4, dtype=torch.float64, device=X.device)
    nbytes = int(_capi.lib().flr_minmax_workspace(K, P, nmal))
    ws, wp = _ws(nbytes, X.device)
    _capi.call("flr_minmax_rows", X.data_ptr(), K, P, ldx, nmal, int(objective), int(perturb), _ptr(global_flat),
               gamma.data_ptr(), _ptr(stats), wp, nbytes, _stream(X))
    if not diagnostics:
        return gamma
    off = wp - ws.data_ptr()
    sig = off + (4 * P + 255) // 256 * 256
    return (gamma, stats, ws[off:off + 4 * P].view(torch.float32).clone(),
            ws[sig:sig + 4 * P].view(torch.float32).clone())


REPLACE_NONE, REPLACE_NORM, REPLACE_DISTANCE = 0, 1, 2  # FLR_REPLACE_* (mode)
REPLACE_MEDIAN, REPLACE_MAX, REPLACE_MEAN = 0, 1, 2      # FLR_REPLACE_* (stat)
REPLACE_MAX_CLIENTS = 1024  # flr_replace_strength's limit


def _positive_finite(value, name: str) -> float:
    """value as a float, a finite number > 0 (a bool or a string is not one)."""
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not 0.0 < float(value) < float("inf"):
        raise ValueError(f"{name} must be a finite number > 0, got {value!r}")
    return float(value)


def replace_strength(norms: Optional[torch.Tensor], G: Optional[torch.Tensor], f: int, boost: float,
                     mode: int = REPLACE_NONE, stat: int = REPLACE_MEDIAN, rho: float = 1.0,
                     K: Optional[int] = None, device=None):
    """Model replacement's strengths (flr_replace_strength; the arithmetic in
    include/flr.h): gamma_i of the attackers 0..f-1, boost cut back to rho times
    a statistic of the benign rows' norms (REPLACE_NORM: stat REPLACE_MEDIAN /
    REPLACE_MAX / REPLACE_MEAN) or to rho times their largest mutual distance
    (REPLACE_DISTANCE).  norms: float64 [K], row_norms(X, center=g) (None in
    REPLACE_NONE, optional in REPLACE_DISTANCE); G: float64 [K, K],
    rows_gram(X, center=g) (REPLACE_DISTANCE only).  K and device are taken from
    norms or G, or given (REPLACE_NONE with neither).  Returns (gamma64 float64
    [f], gamma32 float32 [f], status int32 [f] — 0 boost-limited, 1
    bound-limited, 2 infeasible, 3 left alone —, flags int32 [1]: bit 0 a
    non-finite benign statistic, bit 1 a non-finite attacker) as device tensors;
    no host synchronisation."""
    f, mode, stat = int(f), int(mode), int(stat)
    boost, rho = _positive_finite(boost, "boost"), _positive_finite(rho, "rho")
    if mode not in (REPLACE_NONE, REPLACE_NORM, REPLACE_DISTANCE):
        raise ValueError(f"unknown replace_strength mode {mode}")
    if stat not in (REPLACE_MEDIAN, REPLACE_MAX, REPLACE_MEAN):
        raise ValueError(f"unknown replace_strength stat {stat}")
    for name, t in (("norms", norms), ("G", G)):
        if t is not None:
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError(f"{name} must be a CUDA/HIP tensor (the engine has no CPU path)")
            K = t.shape[0] if K is None else K
            device = t.device if device is None else device
    if K is None or device is None:
        raise ValueError("replace_strength needs norms, G, or K and device")
    K, device = int(K), torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("replace_strength runs on a CUDA/HIP device (the engine has no CPU path)")
    if not 1 <= f < K:
        raise ValueError(f"replace_strength needs 1 <= f < K (got f = {f}, K = {K})")
    if K > REPLACE_MAX_CLIENTS:
        raise ValueError(f"replace_strength handles at most {REPLACE_MAX_CLIENTS} clients, got {K}")
    if norms is not None:
        _check_vector(norms, K, device, "norms", torch.float64)
    if G is not None and (G.device != device or G.dtype != torch.float64 or tuple(G.shape) != (K, K)
                          or not G.is_contiguous()):
        raise ValueError(f"G must be a contiguous float64 [{K}, {K}] matrix on {device}")
    if mode == REPLACE_NORM and norms is None:
        raise ValueError("REPLACE_NORM needs norms")
    if mode == REPLACE_DISTANCE:
        if G is None:
            raise ValueError("REPLACE_DISTANCE needs G")
        if K - f < 2:
            raise ValueError(f"REPLACE_DISTANCE needs two benign rows (got K - f = {K - f})")
    gamma64 = torch.empty(f, dtype=torch.float64, device=device)
    gamma32 = torch.empty(f, dtype=torch.float32, device=device)
    status = torch.empty(f, dtype=torch.int32, device=device)
    flags = torch.empty(1, dtype=torch.int32, device=device)
    _capi.call("flr_replace_strength", _ptr(norms), _ptr(G), K, f, boost, mode, stat, rho, gamma64.data_ptr(),
               gamma32.data_ptr(), status.data_ptr(), flags.data_ptr(), _stream(gamma64))
    return gamma64, gamma32, status, flags


def scale_rows_from(X: torch.Tensor, center: torch.Tensor, gamma32: torch.Tensor) -> torch.Tensor:
    """In place (flr_scale_rows_from): rows i < n = len(gamma32) of X <- center +
    (X_i - center) * gamma32[i], three separately rounded fp32 operations; a row
    with gamma32[i] == 1 or NaN is neither read nor written.  center: float32
    [P], gamma32: float32 [n], n <= K, on X's device.  Returns X."""
    K, P, ldx = _check_matrix(X)
    if K < 1 or P < 1:
        raise ValueError(f"scale_rows_from needs K >= 1 and P >= 1, got {K} x {P}")
    _check_vector(center, P, X.device, "center")
    n = gamma32.numel() if isinstance(gamma32, torch.Tensor) else -1
    if n > K:
        raise ValueError(f"gamma32 has {n} entries for {K} rows")
    _check_vector(gamma32, n, X.device, "gamma32")
    _capi.call("flr_scale_rows_from", X.data_ptr(), K, P, ldx, center.data_ptr(), gamma32.data_ptr(), n, _stream(X))
    return X


FANG_THRESHOLD = 1e-5        # FLR_FANG_THRESHOLD, the paper's
FANG_MAX_BENIGN = 1024       # flr_fang_krum_*'s limit on K - f


def _fang_krum_shape(K: int, f: int, threshold) -> Tuple[int, int, float]:
    """(K, f, threshold) of the Krum attack checked on the host."""
    K, f = int(K), int(f)
    threshold = _positive_finite(threshold, "threshold")
    if f < 1 or K < 2 * f + 3:
        raise ValueError(f"the Krum attack needs f >= 1 and Krum's own K >= 2f + 3 (got K = {K}, f = {f})")
    if K - f > FANG_MAX_BENIGN:
        raise ValueError(f"the Krum attack handles at most {FANG_MAX_BENIGN} benign rows, got {K - f}")
    return K, f, threshold


def fang_krum_strength(G: torch.Tensor, b: torch.Tensor, c: torch.Tensor, K: int, f: int,
                       threshold: float = FANG_THRESHOLD):
    """The Krum attack's strength (flr_fang_krum_strength; the arithmetic in
    include/flr.h): the largest lambda = lambda0 * 2^-t for which Krum picks a row
    g - lambda * s, from the benign rows' centered Gram matrix G (float64 [K - f,
    K - f], rows_gram(X[f:], center=g)), b (float64 [K - f], b_i = <s, x_i - g>)
    and c (float64 scalar or [1], <s, s>).  Returns (lambda64 float64 scalar,
    lambda32 float32 scalar, info int32 [2] — status (0 found, 1 threshold
    reached, 2 no direction, 3 not finite) and t —, stats float64 [5]: lambda0,
    T, E, the last probe's S_att and S_min) as device tensors; no host
    synchronisation."""
    K, f, threshold = _fang_krum_shape(K, f, threshold)
    nb = K - f
    if not isinstance(G, torch.Tensor) or not G.is_cuda:
        raise RuntimeError("G must be a CUDA/HIP tensor (the engine has no CPU path)")
    if G.dtype != torch.float64 or tuple(G.shape) != (nb, nb) or not G.is_contiguous():
        raise ValueError(f"G must be a contiguous float64 [{nb}, {nb}] matrix")
    _check_vector(b, nb, G.device, "b", torch.float64)
    _check_vector(c, 1, G.device, "c", torch.float64)
    lam64 = torch.empty((), dtype=torch.float64, device=G.device)
    lam32 = torch.empty((), dtype=torch.float32, device=G.device)
    info = torch.empty(2, dtype=torch.int32, device=G.device)
    stats = torch.empty(5, dtype=torch.float64, device=G.device)
    nbytes = int(_capi.lib().flr_fang_krum_strength_workspace(K, f))
    ws, wp = _ws(nbytes, G.device)
    _capi.call("flr_fang_krum_strength", G.data_ptr(), b.data_ptr(), c.data_ptr(), K, f, threshold, lam64.data_ptr(),
               lam32.data_ptr(), info.data_ptr(), stats.data_ptr(), wp, nbytes, _stream(G))
    return lam64, lam32, info, stats


def fang_krum_rows(X: torch.Tensor, nmal: int, global_flat: torch.Tensor, threshold: float = FANG_THRESHOLD,
                   diagnostics: bool = False):
    """Fang et al.'s Krum attack in place (flr_fang_krum_rows): rows [0, nmal) of
    X <- g - lambda * s, g = global_flat, s = sign(mu - g) of the benign rows'
    [nmal, K) mean, lambda the largest lambda0 * 2^-t above threshold for which
    Krum (num_malicious = nmal) picks one of those rows, solved on the device in
    closed form.  The whole call is enqueued on the current stream: no host
    synchronisation.  Returns (lambda float64 device scalar — NaN: a statistic was
    not finite and no row was written —, info int32 [2]: status, t), or with
    diagnostics (lambda, info, stats float64 [nb + 6] — b_i, c, lambda0, T, E,
    S_att, S_min —, G float64 [nb, nb], mu float32 [P], s float32 [P]) as device
    tensors."""
    K, P, ldx = _check_matrix(X)
    K, nmal, threshold = _fang_krum_shape(K, nmal, threshold)
    _check_vector(global_flat, P, X.device, "global_flat")
    nb = K - nmal
    lam = torch.empty((), dtype=torch.float64, device=X.device)
    info = torch.empty(2, dtype=torch.int32, device=X.device)
    stats = G = None
    if diagnostics:
        stats = torch.empty(nb + 6, dtype=torch.float64, device=X.device)
        G = torch.empty((nb, nb), dtype=torch.float64, device=X.device)
    nbytes = int(_capi.lib().flr_fang_krum_workspace(K, P, nmal))
    ws, wp = _ws(nbytes, X.device)
    _capi.call("flr_fang_krum_rows", X.data_ptr(), K, P, ldx, nmal, global_flat.data_ptr(), threshold, lam.data_ptr(),
               info.data_ptr(), _ptr(stats), _ptr(G), wp, nbytes, _stream(X))
    if not diagnostics:
        return lam, info
    off = wp - ws.data_ptr()
    sgn = off + (4 * P + 255) // 256 * 256
    return (lam, info, stats, G, ws[off:off + 4 * P].view(torch.float32).clone(),
            ws[sgn:sgn + 4 * P].view(torch.float32).clone())


def _fang_trim_b(b) -> float:
    """b as the float32 value the kernel gets: a finite number > 1 (a bool or a
    string is not one; the paper uses 2)."""
    ok = not isinstance(b, bool) and isinstance(b, (int, float)) and abs(b) < 2.0 ** 128
    b32 = ctypes.c_float(b).value if ok else 0.0
    if not 1.0 < b32 < float("inf"):
        raise ValueError(f"b must be a finite number > 1 in float32, got {b!r}")
    return b32


def fang_trim_rows(X: torch.Tensor, nmal: int, global_flat: torch.Tensor, b: float = 2.0, seed: int = 0,
                   stream: int = 0, col0: int = 0) -> torch.Tensor:
    """Fang et al.'s trimmed-mean / median attack in place (flr_fang_trim_rows):
    per coordinate, rows [0, nmal) of X <- points drawn just beyond the benign
    rows' [nmal, K) extreme on the side opposite s = sign(mu - g), g =
    global_flat: between the minimum mn and mn / b (mn > 0) or mn * b where s > 0,
    between the maximum mx and mx * b (mx > 0) or mx / b where s < 0, mu where s
    == 0.  The draws are Philox4x32-10 keyed by seed (64 bits) with the counter
    (col0 + column, row, stream): a column range of X called with its own col0
    gives the whole-matrix call's bits; stream (32 bits) is the round index.
    Returns X."""
    K, P, ldx = _check_matrix(X)
    nmal, seed, stream, col0 = int(nmal), int(seed), int(stream), int(col0)
    if not 1 <= nmal < K:
        raise ValueError(f"fang_trim_rows needs 1 <= nmal < K (got nmal = {nmal}, K = {K})")
    _check_vector(global_flat, P, X.device, "global_flat")
    b = _fang_trim_b(b)
    if col0 < 0 or not 0 <= stream < 2 ** 32:
        raise ValueError(f"fang_trim_rows needs col0 >= 0 and 0 <= stream < 2^32 (got {col0}, {stream})")
    _capi.call("flr_fang_trim_rows", X.data_ptr(), K, P, ldx, nmal, global_flat.data_ptr(), b, seed % 2 ** 64, stream,
               col0, _stream(X))
    return X


def centered_clip(X: torch.Tensor, v0: torch.Tensor, tau: float, iters: int, out: Optional[torch.Tensor] = None,
                  diagnostics: bool = False):
    """Centered clipping (flr_centered_clip): from v0, iters times
    v <- v + (1/K) * sum_i (x_i - v) * min(1, tau / ||x_i - v||); tau = 0: the
    threshold of each iteration is the lower median of its K distances.  All
    iterations are enqueued on the current stream: no host synchronisation.
    Returns out (float32 [P]; must not be v0), or with diagnostics (out, norms
    float64 [iters, K], scales float32 [iters, K], taus float32 [iters]) as
    device tensors."""
    K, P, ldx = _check_matrix(X)
    _check_vector(v0, P, X.device, "v0")
    out = _out_vector(out, P, X.device)
    tau, iters = float(tau), int(iters)
    if not tau >= 0.0:
        raise ValueError(f"tau must be >= 0 (0: the median of the distances), got {tau}")
    if iters < 1:
        raise ValueError(f"iters must be >= 1, got {iters}")
    norms = scales = taus = None
    if diagnostics:
        norms = torch.empty((iters, K), dtype=torch.float64, device=X.device)
        scales = torch.empty((iters, K), dtype=torch.float32, device=X.device)
        taus = torch.empty(iters, dtype=torch.float32, device=X.device)
    nbytes = int(_capi.lib().flr_centered_clip_workspace(K, P))
    ws, wp = _ws(nbytes, X.device)
    _capi.call("flr_centered_clip", X.data_ptr(), K, P, ldx, v0.data_ptr(), tau, iters, out.data_ptr(), _ptr(norms),
               _ptr(scales), _ptr(taus), wp, nbytes, _stream(X))
    return (out, norms, scales, taus) if diagnostics else out


DNC_MAX_ITERS, DNC_MAX_POWER_ITERS = 16, 1024  # flr_dnc_select's limits


def dnc_select(X: torch.Tensor, b: int, niters: int, nremove: int, power_iters: int, seed: int = 0,
               cols: Optional[torch.Tensor] = None, diagnostics: bool = False):
    """Divide-and-conquer selection (flr_dnc_select): niters times, b sampled
    columns (generated on the device from seed, or the caller's int64 [niters, b]
    device tensor cols, clamped into range), centered over the rows; every row
    scored by its squared projection on the top singular direction (power_iters
    power steps on the K x K Gram matrix, fp64); the nremove highest scores
    dropped.  keep marks the rows every iteration kept (iteration 0's set, and
    bit 0 of flags, when that intersection is empty).  All iterations are
    enqueued on the current stream: no host synchronisation.  Returns (keep
    int32 [K], count int32 [1]), or with diagnostics (keep, count, scores float64
    [niters, K], cols int64 [niters, b], flags int32 [1]) as device tensors."""
    K, P, ldx = _check_matrix(X)
    b, niters, nremove, power_iters = int(b), int(niters), int(nremove), int(power_iters)
    if not 1 <= b <= P:
        raise ValueError(f"b must be in [1, P = {P}], got {b}")
    if niters < 1 or power_iters < 1:
        raise ValueError(f"niters and power_iters must be >= 1, got {niters} and {power_iters}")
    if not 0 <= nremove <= K - 1:
        raise ValueError(f"nremove must be in [0, K - 1 = {K - 1}], got {nremove}")
    if cols is not None and (not isinstance(cols, torch.Tensor) or cols.device != X.device
                             or cols.dtype != torch.int64 or not cols.is_contiguous()
                             or tuple(cols.shape) != (niters, b)):
        raise ValueError(f"cols must be a contiguous int64 [{niters}, {b}] tensor on {X.device}")
    keep = torch.empty(K, dtype=torch.int32, device=X.device)
    count = torch.empty(1, dtype=torch.int32, device=X.device)
    scores = cols_out = flags = None
    if diagnostics:
        scores = torch.empty((niters, K), dtype=torch.float64, device=X.device)
        cols_out = torch.empty((niters, b), dtype=torch.int64, device=X.device)
        flags = torch.empty(1, dtype=torch.int32, device=X.device)
    nbytes = int(_capi.lib().flr_dnc_workspace(K, b))
    ws, wp = _ws(nbytes, X.device)
    _capi.call("flr_dnc_select", X.data_ptr(), K, P, ldx, b, niters, nremove, power_iters,
               int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(cols), keep.data_ptr(), count.data_ptr(), _ptr(scores),
               _ptr(cols_out), _ptr(flags), wp, nbytes, _stream(X))
    return (keep, count, scores, cols_out, flags) if diagnostics else (keep, count)


def rows_mean_keep(X: torch.Tensor, keep: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The mean of the rows with keep != 0 (flr_rows_mean_keep; keep: int32 [K]
    on X's device, counted there): the bits of rows_mean over the ascending kept
    rows; NaN everywhere when no row is kept.  Only the kept rows are read."""
    K, P, ldx = _check_matrix(X)
    _check_vector(keep, K, X.device, "keep", torch.int32)
    out = _out_vector(out, P, X.device)
    _capi.call("flr_rows_mean_keep", X.data_ptr(), K, P, ldx, keep.data_ptr(), out.data_ptr(), _stream(X))
    return out


FOOLSGOLD_MAX_CLIENTS = 1024  # flr_rows_gram's and flr_foolsgold_weights' limit


def rows_accumulate_(H: torch.Tensor, X: torch.Tensor, center: torch.Tensor) -> torch.Tensor:
    """H += X - center in place (flr_rows_accumulate): per element
    fl(H + fl(X - center)), two fp32 operations.  H, X: [K, P] row-major
    matrices (any row strides), center: [P].  Returns H."""
    K, P, ldh = _check_matrix(H, "H")
    K2, P2, ldx = _check_matrix(X)
    if (K2, P2) != (K, P) or X.device != H.device:
        raise ValueError(f"H is {K} x {P} on {H.device}, X {K2} x {P2} on {X.device}")
    if K < 1 or P < 1:
        raise ValueError(f"rows_accumulate_ needs K >= 1 and P >= 1, got {K} x {P}")
    _check_vector(center, P, H.device, "center")
    _capi.call("flr_rows_accumulate", H.data_ptr(), ldh, X.data_ptr(), ldx, center.data_ptr(), K, P, _stream(H))
    return H


def rows_gram(A: torch.Tensor, center: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float64 [K, K]: G = A A^T over all P coordinates (flr_rows_gram), of the
    rows minus center when one is given (one fp32 subtraction): the products
    exact on the fp64 matrix cores, the fp64 sums in an order fixed by (K, P);
    G is symmetric bit for bit.  K <= 1024."""
    K, P, lda = _check_matrix(A, "A")
    if K < 1 or P < 1:
        raise ValueError(f"rows_gram needs K >= 1 and P >= 1, got {K} x {P}")
    if K > FOOLSGOLD_MAX_CLIENTS:
        raise ValueError(f"rows_gram handles at most {FOOLSGOLD_MAX_CLIENTS} rows, got {K}")
    if center is not None:
        _check_vector(center, P, A.device, "center")
    if out is None:
        out = torch.empty((K, K), dtype=torch.float64, device=A.device)
    elif not isinstance(out, torch.Tensor) or out.device != A.device or out.dtype != torch.float64 \
            or not out.is_contiguous() or tuple(out.shape) != (K, K):
        raise ValueError(f"out must be a contiguous float64 [{K}, {K}] matrix on {A.device}")
    nbytes = int(_capi.lib().flr_rows_gram_workspace(K, P))
    ws, wp = _ws(nbytes, A.device)
    _capi.call("flr_rows_gram", A.data_ptr(), K, P, lda, _ptr(center), out.data_ptr(), wp, nbytes, _stream(A))
    return out


def rows_gram_splits(K: int, P: int) -> int:
    """The column chunks of rows_gram's sum at (K, P) (flr_rows_gram_splits)."""
    return int(_capi.lib().flr_rows_gram_splits(int(K), int(P)))


def foolsgold_weights(G: torch.Tensor, kappa: float = 1.0, diagnostics: bool = False):
    """FoolsGold's client weights from the Gram matrix of the client rows
    (flr_foolsgold_weights; the arithmetic in include/flr.h): alpha float64 [K]
    in [0, 1] and beta = float32(alpha / sum(alpha)), all zero for "no update".
    Returns (alpha, beta), or with diagnostics (alpha, beta, max_cosine float64
    [K], flags int32 [1]: bit 0 no update, bit 1 a row with a non-finite norm)
    as device tensors."""
    if not isinstance(G, torch.Tensor) or not G.is_cuda:
        raise RuntimeError("G must be a CUDA/HIP tensor (the engine has no CPU path)")
    if G.dtype != torch.float64 or G.dim() != 2 or G.shape[0] != G.shape[1] or not G.is_contiguous():
        raise ValueError(f"G must be a contiguous float64 [K, K] matrix (got {G.dtype}, shape {tuple(G.shape)})")
    K = G.shape[0]
    if K < 1:
        raise ValueError("foolsgold_weights needs K >= 1")
    if K > FOOLSGOLD_MAX_CLIENTS:
        raise ValueError(f"foolsgold_weights handles at most {FOOLSGOLD_MAX_CLIENTS} clients, got {K}")
    kappa = float(kappa)
    if not 0.0 < kappa < float("inf"):
        raise ValueError(f"kappa must be a finite number > 0, got {kappa}")
    alpha = torch.empty(K, dtype=torch.float64, device=G.device)
    beta = torch.empty(K, dtype=torch.float32, device=G.device)
    maxcos = flags = None
    if diagnostics:
        maxcos = torch.empty(K, dtype=torch.float64, device=G.device)
        flags = torch.empty(1, dtype=torch.int32, device=G.device)
    _capi.call("flr_foolsgold_weights", G.data_ptr(), K, kappa, alpha.data_ptr(), beta.data_ptr(), _ptr(maxcos),
               _ptr(flags), _stream(G))
    return (alpha, beta, maxcos, flags) if diagnostics else (alpha, beta)


def rows_combine_from(X: torch.Tensor, center: torch.Tensor, beta: torch.Tensor,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = center + sum_i (X_i - center) * beta_i (flr_rows_combine_from): fp32,
    the rows in ascending order, every op separately rounded; rows with beta_i
    == 0 are not read; all beta zero gives center's bits.  beta: float32 [K] on
    X's device.  out must not be center."""
    K, P, ldx = _check_matrix(X)
    if K < 1 or P < 1:
        raise ValueError(f"rows_combine_from needs K >= 1 and P >= 1, got {K} x {P}")
    if K > 4096:
        raise ValueError(f"rows_combine_from handles at most 4096 rows, got {K}")
    _check_vector(center, P, X.device, "center")
    _check_vector(beta, K, X.device, "beta")
    out = _out_vector(out, P, X.device)
    if out.data_ptr() == center.data_ptr():
        raise ValueError("out must not be center")
    _capi.call("flr_rows_combine_from", X.data_ptr(), K, P, ldx, center.data_ptr(), beta.data_ptr(), out.data_ptr(),
               _stream(X))
    return out


FLAME_MAX_CLIENTS = 1024  # flr_rows_gram's and flr_flame_select's limit


def flame_cluster_size(K: int, m=None) -> int:
    """FLAME's min_cluster_size for K clients: K // 2 + 1 (the paper's) for
    None, else an integer with 2 m > K and m <= K."""
    if m is None:
        return K // 2 + 1
    if isinstance(m, bool) or not isinstance(m, int) or m > K or 2 * m <= K:
        raise ValueError(f"min_cluster_size must be None or an integer in [{K // 2 + 1}, {K}] for {K} clients, "
                         f"got {m!r}")
    return m


def flame_select(G: torch.Tensor, m: Optional[int] = None, lam: float = 0.0, norms: Optional[torch.Tensor] = None,
                 diagnostics: bool = False):
    """FLAME's admitted cluster and clipped weights from the Gram matrix of the
    client updates (flr_flame_select; the arithmetic in include/flr.h): the
    first single-linkage component of the cosine distances that reaches m rows
    (default K // 2 + 1) is admitted; S is the lower median of the update norms
    (norms float64 [K] when given, else sqrt(G_ii)); beta_i = float32(min(1, S /
    e_i) / L) for the L admitted rows, 0 for the others; sigma = float32(lam *
    S).  Returns (keep int32 [K], beta float32 [K], sigma float32 [1]), or with
    diagnostics (keep, beta, sigma, stats float64 [3]: S, t*, L, flags int32 [1]:
    bit 0 no cluster, bit 1 a row with a non-finite norm) as device tensors."""
    if not isinstance(G, torch.Tensor) or not G.is_cuda:
        raise RuntimeError("G must be a CUDA/HIP tensor (the engine has no CPU path)")
    if G.dtype != torch.float64 or G.dim() != 2 or G.shape[0] != G.shape[1] or not G.is_contiguous():
        raise ValueError(f"G must be a contiguous float64 [K, K] matrix (got {G.dtype}, shape {tuple(G.shape)})")
    K = G.shape[0]
    if K < 1:
        raise ValueError("flame_select needs K >= 1")
    if K > FLAME_MAX_CLIENTS:
        raise ValueError(f"flame_select handles at most {FLAME_MAX_CLIENTS} clients, got {K}")
    m = flame_cluster_size(K, m)
    lam = float(lam)
    if not 0.0 <= lam < float("inf"):
        raise ValueError(f"lam must be a finite number >= 0, got {lam}")
    if norms is not None:
        _check_vector(norms, K, G.device, "norms", torch.float64)
    keep = torch.empty(K, dtype=torch.int32, device=G.device)
    beta = torch.empty(K, dtype=torch.float32, device=G.device)
    sigma = torch.empty(1, dtype=torch.float32, device=G.device)
    stats = flags = None
    if diagnostics:
        stats = torch.empty(3, dtype=torch.float64, device=G.device)
        flags = torch.empty(1, dtype=torch.int32, device=G.device)
    _capi.call("flr_flame_select", G.data_ptr(), _ptr(norms), K, m, lam, keep.data_ptr(), beta.data_ptr(),
               sigma.data_ptr(), _ptr(stats), _ptr(flags), _stream(G))
    return (keep, beta, sigma, stats, flags) if diagnostics else (keep, beta, sigma)


def add_gaussian_(v: torch.Tensor, sigma: torch.Tensor, seed: int = 0, stream: int = 0, col0: int = 0) -> torch.Tensor:
    """v += sigma * z in place (flr_add_gaussian): z standard normal, Box-Muller
    on Philox4x32-10 keyed by seed (64 bits) with the counter ((col0 + k) >> 2, 0,
    stream): a range of v called with its own col0 gives the whole call's bits;
    stream (32 bits) is the call index.  v: float32 [P] contiguous (any 4-byte
    alignment); sigma: float32 [1] on v's device, 0 leaves v's bits.  Returns v."""
    if not isinstance(v, torch.Tensor) or not v.is_cuda:
        raise RuntimeError("v must be a CUDA/HIP tensor (the engine has no CPU path)")
    if v.dtype != torch.float32 or v.dim() != 1 or not v.is_contiguous():
        raise ValueError(f"v must be a contiguous float32 vector (got {v.dtype}, shape {tuple(v.shape)})")
    _check_vector(sigma, 1, v.device, "sigma")
    seed, stream, col0 = int(seed), int(stream), int(col0)
    if col0 < 0 or col0 + v.numel() > 2 ** 63 - 1 or not 0 <= stream < 2 ** 32:
        raise ValueError(f"add_gaussian_ needs 0 <= col0, col0 + P < 2^63 and 0 <= stream < 2^32 (got {col0}, {stream})")
    if v.numel():  # an empty tensor has no address
        _capi.call("flr_add_gaussian", v.data_ptr(), v.numel(), sigma.data_ptr(), seed % 2 ** 64, stream, col0,
                   _stream(v))
    return v


def _check_rlr(theta: int, eta: float, K: Optional[int]) -> Tuple[int, float]:
    theta, eta = int(theta), float(eta)
    if theta < 0 or (K is not None and theta > K):
        raise ValueError(f"theta must be in [0, K{'' if K is None else f' = {K}'}], got {theta}")
    if not 0.0 < eta < float("inf"):
        raise ValueError(f"eta must be a finite number > 0, got {eta}")
    return theta, eta


def sign_vote(X: torch.Tensor, g: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The clients' per-coordinate sign vote against g (flr_sign_vote): int32 [P],
    #{k : X[k, p] > g[p]} - #{k : X[k, p] < g[p]} — comparisons only, so a NaN
    votes 0 and -0 against +0 votes 0.  g: float32 [P] on X's device."""
    K, P, ldx = _check_matrix(X)
    _check_vector(g, P, X.device, "g")
    out = _out_vector(out, P, X.device, torch.int32)
    _capi.call("flr_sign_vote", X.data_ptr(), K, P, ldx, g.data_ptr(), out.data_ptr(), _stream(X))
    return out


def rlr_apply(agg: torch.Tensor, g: torch.Tensor, votes: torch.Tensor, theta: int, eta: float = 1.0,
              out: Optional[torch.Tensor] = None, count: bool = False):
    """The robust learning rate's step (flr_rlr_apply): per coordinate, with d =
    agg - g, out = g + eta * d where |votes| >= theta (agg's own bits at eta == 1)
    and g - eta * d elsewhere; every op a separately rounded fp32 op.  out may be
    agg (in place), not g.  Returns out, or with count (out, flipped int64 [1]: the
    coordinates whose learning rate was negated) as device tensors."""
    if not isinstance(agg, torch.Tensor) or not agg.is_cuda:
        raise RuntimeError("agg must be a CUDA/HIP tensor (the engine has no CPU path)")
    P = agg.numel()
    _check_vector(agg, P, agg.device, "agg")
    _check_vector(g, P, agg.device, "g")
    _check_vector(votes, P, agg.device, "votes", torch.int32)
    theta, eta = _check_rlr(theta, eta, None)
    out = _out_vector(out, P, agg.device)
    flipped = torch.empty(1, dtype=torch.int64, device=agg.device) if count else None
    _capi.call("flr_rlr_apply", agg.data_ptr(), g.data_ptr(), votes.data_ptr(), P, theta, eta, out.data_ptr(),
               _ptr(flipped), _stream(agg))
    return (out, flipped) if count else out


def rlr_fedavg(X: torch.Tensor, num_examples, g: torch.Tensor, theta: int, eta: float = 1.0,
               out: Optional[torch.Tensor] = None, diagnostics: bool = False):
    """FedAvg under the robust learning rate in one pass over X (flr_rlr_fedavg):
    the bits of fedavg, then sign_vote, then rlr_apply.  Returns out (float32 [P];
    must not be g), or with diagnostics (out, votes int32 [P], flipped int64 [1])
    as device tensors."""
    K, P, ldx = _check_matrix(X)
    n = _examples(num_examples, K, X.device)
    _check_vector(g, P, X.device, "g")
    theta, eta = _check_rlr(theta, eta, K)
    out = _out_vector(out, P, X.device)
    votes = flipped = None
    if diagnostics:
        votes = torch.empty(P, dtype=torch.int32, device=X.device)
        flipped = torch.empty(1, dtype=torch.int64, device=X.device)
    _capi.call("flr_rlr_fedavg", X.data_ptr(), K, P, ldx, n.data_ptr(), g.data_ptr(), theta, eta, out.data_ptr(),
               _ptr(votes), _ptr(flipped), _stream(X))
    return (out, votes, flipped) if diagnostics else out


SPARSEFED_MAX_CLIENTS = 4096  # flr_sparsefed_weights' and flr_sparsefed_accumulate's limit
TOPK_BINS = 2048              # the level-1 histogram of flr_topk_abs_select
# The select's scratch, kept per (device, stream) like the reference distances': a
# mask or apply call reads what the last select on that device and stream left.
_TOPK_WS: Dict[Tuple[int, int], torch.Tensor] = {}


def _topk_workspace(P: int, device, stream: int) -> Tuple[int, int]:
    nbytes = int(_capi.lib().flr_topk_abs_workspace(P))
    index = torch.device(device).index
    key = (torch.cuda.current_device() if index is None else index, stream)
    ws = _TOPK_WS.get(key)
    if ws is None or ws.numel() < nbytes + 256:
        _TOPK_WS.pop(key, None)
        ws = torch.empty(max(nbytes, 256) + 256, dtype=torch.uint8, device=device)
        _TOPK_WS[key] = ws
    return ws.data_ptr() + (-ws.data_ptr()) % 256, nbytes


def _check_topk_vector(v, name: str) -> int:
    if not isinstance(v, torch.Tensor) or not v.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA/HIP tensor (the engine has no CPU path)")
    if v.dtype != torch.float32 or v.dim() != 1 or not v.is_contiguous():
        raise ValueError(f"{name} must be a contiguous float32 vector (got {v.dtype}, shape {tuple(v.shape)})")
    if v.numel() >= 2 ** 32:
        raise ValueError(f"{name} holds {v.numel()} coordinates, the select's counts are 32-bit")
    return v.numel()


def sparsefed_weights(norms: torch.Tensor, clip_norm: Optional[float] = None, diagnostics: bool = False):
    """SparseFed's clipped weights from the clients' update norms
    (flr_sparsefed_weights; the arithmetic in include/flr.h): with n the rows
    whose norm is finite and L = clip_norm, or for None the lower median of those
    rows' norms, beta_i = float32(min(1, L / e_i) / n), exactly 0 for a row with a
    non-finite norm.  norms: float64 [K].  Returns beta float32 [K], or with
    diagnostics (beta, stats float64 [3]: L, n, the rows clipped, flags int32 [1]:
    bit 0 no good row, bit 1 a bad row) as device tensors."""
    if not isinstance(norms, torch.Tensor) or not norms.is_cuda:
        raise RuntimeError("norms must be a CUDA/HIP tensor (the engine has no CPU path)")
    K = norms.numel()
    _check_vector(norms, K, norms.device, "norms", torch.float64)
    if K < 1:
        raise ValueError("sparsefed_weights needs K >= 1")
    if K > SPARSEFED_MAX_CLIENTS:
        raise ValueError(f"sparsefed_weights handles at most {SPARSEFED_MAX_CLIENTS} clients, got {K}")
    clip = 0.0
    if clip_norm is not None:
        clip = float(clip_norm)
        if not 0.0 < clip < float("inf"):
            raise ValueError(f"clip_norm must be None or a finite number > 0, got {clip_norm!r}")
    beta = torch.empty(K, dtype=torch.float32, device=norms.device)
    stats = flags = None
    if diagnostics:
        stats = torch.empty(3, dtype=torch.float64, device=norms.device)
        flags = torch.empty(1, dtype=torch.int32, device=norms.device)
    _capi.call("flr_sparsefed_weights", norms.data_ptr(), K, clip, beta.data_ptr(), _ptr(stats), _ptr(flags),
               _stream(norms))
    return (beta, stats, flags) if diagnostics else beta


def sparsefed_accumulate_(X: torch.Tensor, g: torch.Tensor, beta: torch.Tensor, W: torch.Tensor,
                          U: Optional[torch.Tensor] = None, rho: float = 0.0, diagnostics: bool = False):
    """W += [rho * U +] sum_i (X_i - g) * beta_i in place (flr_sparsefed_accumulate):
    fp32, the rows in ascending order, every op separately rounded; rows with
    beta_i == 0 are not read; with rho != 0, U <- rho * U + the sum first.  A
    coordinate whose new W is not finite is set to +0 (U too) and counted.  W, U:
    float32 [P] on X's device (U only with rho != 0).  Returns W, or with
    diagnostics (W, hist uint32-as-int32 [2048]: the level-1 histogram of W's
    keys for topk_abs_select, dropped int64 [1]) as device tensors."""
    K, P, ldx = _check_matrix(X)
    if K < 1:
        raise ValueError("sparsefed_accumulate_ needs K >= 1")
    if K > SPARSEFED_MAX_CLIENTS:
        raise ValueError(f"sparsefed_accumulate_ handles at most {SPARSEFED_MAX_CLIENTS} rows, got {K}")
    rho = float(rho)
    if not 0.0 <= rho < 1.0:
        raise ValueError(f"rho must be in [0, 1), got {rho}")
    _check_vector(g, P, X.device, "g")
    _check_vector(beta, K, X.device, "beta")
    _check_vector(W, P, X.device, "W")
    if rho != 0.0:
        _check_vector(U, P, X.device, "U")
    hist = dropped = None
    if diagnostics:
        hist = torch.empty(TOPK_BINS, dtype=torch.int32, device=X.device)
        dropped = torch.empty(1, dtype=torch.int64, device=X.device)
        if P == 0:
            hist.zero_()
            dropped.zero_()
    if P:  # an empty tensor has no address
        _capi.call("flr_sparsefed_accumulate", X.data_ptr(), K, P, ldx, g.data_ptr(), beta.data_ptr(), rho,
                   W.data_ptr(), _ptr(U) if rho != 0.0 else None, _ptr(hist), _ptr(dropped), _stream(X))
    return (W, hist, dropped) if diagnostics else W


def topk_abs_select(v: torch.Tensor, k: int, hist: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The exact magnitude top-k of v (flr_topk_abs_select): a three-digit radix
    select on key = bits & 0x7fffffff (a NaN or an inf ranks with zero).  Returns
    sel, int32 [4] on the device holding the uint32 words T (the k-th largest
    key), n_gt (the keys above it), r (how many of the keys == T are selected: the
    lowest indices) and the flags (bit 0: v holds a NaN or an inf).  hist: the
    level-1 histogram of v's keys when sparsefed_accumulate_ counted it.  The
    scratch topk_abs_mask / sparsefed_apply_ read is kept per device and stream:
    call them before the next select there."""
    P = _check_topk_vector(v, "v")
    k = int(k)
    if not 1 <= k <= P:
        raise ValueError(f"k must be in [1, {P}], got {k}")
    if hist is not None:
        _check_vector(hist, TOPK_BINS, v.device, "hist", torch.int32)
    sel = torch.empty(4, dtype=torch.int32, device=v.device)
    wp, nbytes = _topk_workspace(P, v.device, _stream(v))
    _capi.call("flr_topk_abs_select", v.data_ptr(), P, k, _ptr(hist), sel.data_ptr(), wp, nbytes, _stream(v))
    return sel


def topk_abs_mask(v: torch.Tensor, sel: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [P]: 1 where topk_abs_select(v, k) selected the coordinate
    (flr_topk_abs_mask), from sel and that call's scratch."""
    P = _check_topk_vector(v, "v")
    if P < 1:
        raise ValueError("topk_abs_mask needs P >= 1")
    _check_vector(sel, 4, v.device, "sel", torch.int32)
    out = _out_vector(out, P, v.device, torch.uint8)
    wp, nbytes = _topk_workspace(P, v.device, _stream(v))
    _capi.call("flr_topk_abs_mask", v.data_ptr(), P, sel.data_ptr(), wp, nbytes, out.data_ptr(), _stream(v))
    return out


def sparsefed_apply_(g: torch.Tensor, W: torch.Tensor, sel: torch.Tensor, U: Optional[torch.Tensor] = None,
                     out: Optional[torch.Tensor] = None, mask: bool = False):
    """out = g + W on the coordinates topk_abs_select(W, k) selected, where W (and
    U when given) become +0; g's bits elsewhere (flr_sparsefed_apply).  out must
    not be g or W.  Returns out, or with mask (out, mask uint8 [P])."""
    P = _check_topk_vector(W, "W")
    if P < 1:
        raise ValueError("sparsefed_apply_ needs P >= 1")
    _check_vector(g, P, W.device, "g")
    if U is not None:
        _check_vector(U, P, W.device, "U")
    _check_vector(sel, 4, W.device, "sel", torch.int32)
    out = _out_vector(out, P, W.device)
    m = torch.empty(P, dtype=torch.uint8, device=W.device) if mask else None
    wp, nbytes = _topk_workspace(P, W.device, _stream(W))
    _capi.call("flr_sparsefed_apply", g.data_ptr(), W.data_ptr(), _ptr(U), P, sel.data_ptr(), wp, nbytes,
               out.data_ptr(), _ptr(m), _stream(W))
    return (out, m) if mask else out


def row_norms(X: torch.Tensor, center: Optional[torch.Tensor] = None, kind: str = "l2") -> torch.Tensor:
    """float64 [K]: ||X_i - center|| per row (l2 or linf); fp32 differences,
    fp64 accumulation in a fixed order (differential_privacy.py:223-236,
    trimmed_mean.py:234)."""
    K, P, ldx = _check_matrix(X)
    if kind not in ("l2", "linf"):
        raise ValueError(f"unknown norm kind {kind!r}")
    if center is not None:
        center = center.contiguous()  # a strided view is accepted
        _check_vector(center, P, X.device, "center")
    out = torch.empty(K, dtype=torch.float64, device=X.device)
    nbytes = int(_capi.lib().flr_row_norms_workspace(K))
    ws, wp = _ws(nbytes, X.device)
    _capi.call("flr_row_norms", X.data_ptr(), K, P, ldx, _ptr(center), 0 if kind == "l2" else 1, out.data_ptr(),
               wp, nbytes, _stream(X))
    return out


def row_dots(X: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """float64 [K]: X_i . v (fltrust.py:176), exact products, fp64 fixed-order sum."""
    K, P, ldx = _check_matrix(X)
    v = v.contiguous()  # a strided view is accepted
    _check_vector(v, P, X.device, "v")
    out = torch.empty(K, dtype=torch.float64, device=X.device)
    nbytes = int(_capi.lib().flr_row_norms_workspace(K))
    ws, wp = _ws(nbytes, X.device)
    _capi.call("flr_row_dots", X.data_ptr(), K, P, ldx, v.data_ptr(), out.data_ptr(), wp, nbytes, _stream(X))
    return out


def weighted_rows(X: torch.Tensor, weights, divisor: float, rows=None, scales=None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = (sum_j fl(fl(X[rows[j]] * scales[j]) * weights[j])) / divisor, in j order
    (the Python-sum weighted averages of differential_privacy.py:141-148, 268-276,
    323-330 and trimmed_mean.py:240)."""
    K, P, ldx = _check_matrix(X)
    w = torch.as_tensor(weights, dtype=torch.float32).to(X.device).contiguous()
    m = w.numel()
    r = None
    if rows is not None:
        r = torch.as_tensor(rows, dtype=torch.int32).to(X.device).contiguous()
        if r.numel() != m:
            raise ValueError("rows and weights differ in length")
    elif m != K:
        raise ValueError(f"{m} weights for {K} rows")
    s = None
    if scales is not None:
        s = torch.as_tensor(scales, dtype=torch.float32).to(X.device).contiguous()
        if s.numel() != m:
            raise ValueError("scales and weights differ in length")
    out = _out_vector(out, P, X.device, name=None)
    _capi.call("flr_weighted_rows", X.data_ptr(), K, P, ldx, _ptr(r), m, w.data_ptr(), _ptr(s), float(divisor),
               out.data_ptr(), _stream(X))
    return out


# ---- coordinate-sharded Krum distances (flr_pairwise_* phases, include/flr.h) ----

# The reference-exact distances' workspace (the chain sums and the chain-major
# copy of X, up to 8 GiB per segment: ~6 GB at C3) is kept per (device,
# stream) and reused by every later call that fits in it, instead of being
# allocated per call.  FLR_REF_WS_CAP (bytes) bounds it: the
# library then runs the chains over more, shorter segments (the same D).
REF_WS_CAP = int(os.environ.get("FLR_REF_WS_CAP", "0")) or None
_REF_WS: Dict[Tuple[int, int], torch.Tensor] = {}


def _ref_workspace(K: int, P: int, device, stream: int) -> Tuple[int, int]:
    nbytes = int(_capi.lib().flr_pairwise_l2_reference_workspace(K, P))
    if REF_WS_CAP is not None:
        nbytes = min(nbytes, REF_WS_CAP)
    key = (torch.device(device).index or 0, stream)
    ws = _REF_WS.get(key)
    if ws is None or ws.numel() < nbytes + 256:
        _REF_WS.pop(key, None)
        ws = torch.empty(max(nbytes, 256) + 256, dtype=torch.uint8, device=device)
        _REF_WS[key] = ws
    return ws.data_ptr() + (-ws.data_ptr()) % 256, nbytes


def release_workspaces() -> None:
    """Drop the cached reference-exact and top-k workspaces (their HBM returns to torch's allocator)."""
    _REF_WS.clear()
    _TOPK_WS.clear()


def pairwise_l2_reference_sharded(cs, tap_blocks=None) -> torch.Tensor:
    """The reference-exact distances (pairwise_l2 "reference") from coordinate
    slices (flr.shard.CoordSlice, the reference's coordinate order): the
    chains run through the ranks in order — rank r continues every pair's 8
    chains over its coordinate range from where rank r-1 left them (the
    8·K² fp32 sums passed on), the last rank adds the P mod 8 tail and takes
    the square roots, and D is broadcast.  Each chain step is the same fp32
    operation in the same order as on one GPU, so D is bit-identical to
    pairwise_l2(X, "reference") at every world size.  A chain cannot be split,
    so the ranks run one after another: the phase costs about the one-GPU
    chain time at any G, with only this rank's 1/G of the rows transposed.
    tap_blocks (a training-order round): the matrix's tap-major blocks
    [(off, Cout, Cin, KK), ...]; the rank boundaries must not cut one
    (shard.aligned_bounds), and the blocks inside this slice are read in
    place (flr_pairwise_l2_reference_partial_tap)."""
    lib = _capi.lib()
    K, P, dev = cs.K, cs.P, cs.data.device
    X, ld = cs.data, cs.data.stride(0)
    comm, rank, world = cs.comm, cs.comm.rank, cs.comm.world
    R = P // 8
    full_end = min(cs.end, 8 * R)
    steps = max(0, full_end - cs.begin) // 8
    if cs.begin % 8:
        raise ValueError("coordinate slices must start at a multiple of 8 coordinates")
    if X.data_ptr() % 16 or ld % 4:
        raise ValueError("coordinate slice rows must be 16-B aligned")
    taps = []
    for o, co, ci, kk in (tap_blocks or ()):
        e = o + co * ci * kk
        if e <= cs.begin or o >= cs.end:
            continue
        if o < cs.begin or e > cs.begin + 8 * steps:
            raise ValueError(f"tap block [{o}, {e}) crosses this rank's chain range [{cs.begin}, "
                             f"{cs.begin + 8 * steps}): the rank boundaries must be tap-block aligned")
        taps += [o - cs.begin, co, ci, kk]
    tarr = (ctypes.c_int64 * max(1, len(taps)))(*taps)
    nbytes = int(lib.flr_pairwise_l2_reference_workspace(K, 8 * steps))
    ws, wp = _ws(nbytes, dev)
    st = _stream(X)
    A = torch.empty(0, dtype=torch.float32, device=dev)
    if K > 1:
        A = torch.as_strided(ws, (8 * K * K * 4,), (1,), (wp - ws.data_ptr())).view(torch.float32)
        if rank > 0:
            comm.recv(A, rank - 1)
        _capi.call("flr_pairwise_l2_reference_partial_tap", X.data_ptr(), K, steps, ld, ctypes.addressof(tarr),
                   len(taps) // 4, int(rank == 0), wp, nbytes, st)
        if rank < world - 1:
            comm.send(A, rank + 1)
    D = torch.empty((K, K), dtype=torch.float64, device=dev)
    if rank == world - 1:
        ntail = P - 8 * R
        xt = X.data_ptr() + 4 * (8 * R - cs.begin)
        _capi.call("flr_pairwise_l2_reference_finish", xt, K, ntail, ld, int(R > 0), wp, D.data_ptr(), st)
    comm.broadcast(D, world - 1)
    return D


def pairwise_l2_sharded(cs, events=None) -> torch.Tensor:
    """K×K float64 distances from a coordinate slice (flr.shard.CoordSlice):
    every rank ends with the same D, bit-identical to pairwise_l2 on the
    whole matrix.  Collectives: one exact sum of the pivot sample, one exact
    sum of the tail term, one all-gather of the per-slice Gram sums."""
    if cs.plan.bounds is not None:
        raise ValueError("the Gram path's per-slice records need the canonical rank boundaries "
                         "(this slice's are tap-block aligned: a training-order reference-exact round)")
    lib = _capi.lib()
    K, P, dev = cs.K, cs.P, cs.data.device
    X, ld = cs.data, cs.data.stride(0)
    st = _stream(X)
    c0, c1 = cs.plan.chunks(cs.rank)
    S = int(lib.flr_pairwise_sample_len(P))
    D = torch.empty((K, K), dtype=torch.float64, device=dev)
    tail = torch.empty((K, K), dtype=torch.float64, device=dev)
    # tail: coordinates past the last full chunk (held by the last rank)
    t0 = (P // CHUNK) * CHUNK - cs.begin
    t0 = min(max(t0, 0), cs.n)
    _capi.call("flr_pairwise_tail", X.data_ptr(), K, ld, t0, cs.n, tail.data_ptr(), st)
    if S == 0:  # no full chunk anywhere: the tail is everything
        cs.comm.all_reduce_sum(tail)
        gsum = torch.zeros(PW_SLICES * int(lib.flr_pairwise_gsum_len(K)), dtype=torch.float64, device=dev)
        _capi.call("flr_pairwise_finish", gsum.data_ptr(), tail.data_ptr(), K, D.data_ptr(), st)
        return D
    Xs = torch.empty((K, S), dtype=torch.float32, device=dev)
    _capi.call("flr_pairwise_sample", X.data_ptr(), K, ld, P, c0, c1, Xs.data_ptr(), st)
    cs.comm.all_reduce_sum(Xs)
    nsl = cs.q1 - cs.q0
    nbytes = int(lib.flr_pairwise_sliced_workspace(K, P, nsl))
    ws, wp = _ws(nbytes, dev)
    pivot = torch.empty(int(lib.flr_pairwise_pivot_len()), dtype=torch.int32, device=dev)  # the pivot record
    _capi.call("flr_pairwise_pivot", Xs.data_ptr(), K, P, pivot.data_ptr(), wp, nbytes, st)
    glen = int(lib.flr_pairwise_gsum_len(K))
    mine = torch.empty(nsl * glen, dtype=torch.float64, device=dev)
    ev = (None, None) if events is None else events
    _capi.call("flr_pairwise_gram_slices", X.data_ptr(), K, ld, P, cs.q0, cs.q1, pivot.data_ptr(), mine.data_ptr(),
               wp, nbytes, st, ev[0], ev[1])
    cs.comm.all_reduce_sum(tail)
    gsum = torch.empty(PW_SLICES * glen, dtype=torch.float64, device=dev)
    cs.comm.all_gather(gsum, mine)
    _capi.call("flr_pairwise_finish", gsum.data_ptr(), tail.data_ptr(), K, D.data_ptr(), st)
    return D
