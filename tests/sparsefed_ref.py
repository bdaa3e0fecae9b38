"""CPU restatement of SparseFed and the magnitude top-k as include/flr.h fixes
them (flr_sparsefed_weights, flr_sparsefed_accumulate, flr_topk_abs_select,
flr_topk_abs_mask, flr_sparsefed_apply), in numpy: float32 operations one at a
time in client order, float64 for the weights, a stable argsort for the
selection.  It shares no code with the library's Python.  The update norms are
an input (flr_row_norms is an existing call with its own tests): a GPU test
hands over the device's, a host test norms() below."""
from typing import NamedTuple, Optional

import numpy as np

F32_INF_BITS = 0x7F800000
BINS1 = 2048


def f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def bits(a):
    return f32(a).view(np.uint32)


def same_bits(a, b):
    """Two float32 vectors equal bit for bit (tensors or arrays)."""
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else a
    b = b.detach().cpu().numpy() if hasattr(b, "detach") else b
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def norms(X, g):
    """||x_i - g|| in float64 of the float32 differences (a host stand-in for
    flr_row_norms); X may carry padding columns past g's length."""
    with np.errstate(all="ignore"):
        d = (f32(X)[:, :f32(g).size] - f32(g)).astype(np.float64)
        return np.sqrt((d * d).sum(axis=1))


# ---- step 2: the weights ----

class Weights(NamedTuple):
    beta: np.ndarray   # float32 [K]
    L: float
    n: int
    clipped: int
    flags: int


def weights(e, clip_norm: Optional[float] = None) -> Weights:
    e = np.asarray(e, dtype=np.float64)
    K = e.size
    good = np.isfinite(e)
    n = int(good.sum())
    flags = (1 if n == 0 else 0) | (2 if n < K else 0)
    beta = np.zeros(K, dtype=np.float32)
    if n == 0:
        return Weights(beta, 0.0, 0, 0, flags)
    L = float(clip_norm) if clip_norm is not None else float(np.sort(e[good], kind="stable")[(n - 1) // 2])
    clipped = 0
    for i in range(K):
        if not good[i]:
            continue
        if e[i] > L:
            gamma = np.float64(L) / e[i]
            clipped += 1
        else:
            gamma = np.float64(1.0)
        beta[i] = np.float32(gamma / np.float64(n))
    return Weights(beta, L, n, clipped, flags)


# ---- step 3: the accumulation ----

def accumulate(X, g, beta, W, U=None, rho: float = 0.0):
    """(W', U', dropped, hist1): new arrays, the inputs are left alone; U' is
    None at rho == 0."""
    X, g, W = f32(X), f32(g), f32(W)
    with np.errstate(all="ignore"):
        a = np.zeros(g.shape, dtype=np.float32)
        for i in range(X.shape[0]):
            if beta[i] != 0:
                a = a + (X[i] - g) * np.float32(beta[i])
        if rho != 0.0:
            u = np.float32(rho) * f32(U)
            u = u + a
        else:
            u = a
        w = W + u
    bad = ~np.isfinite(w)
    w = np.where(bad, np.float32(0.0), w).astype(np.float32)
    if rho != 0.0:
        u = np.where(bad, np.float32(0.0), u).astype(np.float32)
    hist = np.bincount(keys(w) >> 20, minlength=BINS1).astype(np.int64)
    return w, (u if rho != 0.0 else None), int(bad.sum()), hist


# ---- step 4: the selection ----

def keys(v):
    u = bits(v) & np.uint32(0x7FFFFFFF)
    return np.where(u < F32_INF_BITS, u, np.uint32(0)).astype(np.uint32)


def order(v):
    """The coordinates by descending key, equal keys by ascending index."""
    return np.argsort(-keys(v).astype(np.int64), kind="stable")


class Selection(NamedTuple):
    T: int
    n_gt: int
    r: int
    flags: int
    mask: np.ndarray   # uint8 [P]


def select(v, k: int, by=None) -> Selection:
    """by: order(v), when the caller selects several k on one vector."""
    key = keys(v)
    by = order(v) if by is None else by
    P = key.size
    assert 1 <= k <= P
    mask = np.zeros(P, dtype=np.uint8)
    mask[by[:k]] = 1
    T = int(key[by[k - 1]])
    n_gt = int((key > T).sum())
    flags = 0 if bool(np.isfinite(f32(v)).all()) else 1
    return Selection(T, n_gt, k - n_gt, flags, mask)


# ---- step 5: the apply ----

def apply(g, W, U, mask):
    """(out, W', U'): new arrays."""
    g, W = f32(g), f32(W)
    s = mask.astype(bool)
    with np.errstate(all="ignore"):
        out = np.where(s, g + W, g).astype(np.float32)
    W2 = np.where(s, np.float32(0.0), W).astype(np.float32)
    U2 = None if U is None else np.where(s, np.float32(0.0), f32(U)).astype(np.float32)
    return out, W2, U2


# ---- the defense ----

class Round(NamedTuple):
    out: np.ndarray
    weights: Weights
    dropped: int
    w: np.ndarray        # W after step 3, before the apply
    selection: Selection


class SparseFed:
    """The rule with its state, as SparseFedDefense keeps it."""

    def __init__(self, k: int, clip_norm: Optional[float] = None, rho: float = 0.0):
        self.k, self.clip_norm, self.rho = k, clip_norm, rho
        self.W = self.U = None

    def step(self, X, g, e) -> Round:
        """X [K, P], g [P], e: the K update norms (float64)."""
        P = f32(g).size
        if self.W is None:
            self.W = np.zeros(P, dtype=np.float32)
            self.U = np.zeros(P, dtype=np.float32) if self.rho != 0.0 else None
        wt = weights(e, self.clip_norm)
        w, u, dropped, _ = accumulate(X, g, wt.beta, self.W, self.U, self.rho)
        s = select(w, self.k)
        out, self.W, self.U = apply(g, w, u, s.mask)
        return Round(out, wt, dropped, w, s)


# ---- the tests' inputs (shared by the host guards and the GPU tests) ----

CHUNK = 1024  # the select's chunk of coordinates (include/flr.h)
TOPK_SIZES = (1, 3, 4, 1027, 5000, 262147, 4200003)
TOPK_KINDS = ("randn", "equal", "sparse", "ties", "d3", "d2", "extremes", "nonfinite")
# test_gpu_robust_lr.py's (K, P, ldx - P)
SHAPES = [(1, 5, 3), (2, 1, 3), (5, 7, 2), (16, 5000, 24), (33, 1027, 1), (130, 300, 0)]
FILL = -77.0  # the padding columns' content
ROUNDS = 3
K_FRACTION = 0.05


def topk_ks(P):
    return sorted({k for k in (1, 2, P // 3, P - 1, P) if 1 <= k <= P})


def topk_input(kind: str, P: int, seed: int = 0) -> np.ndarray:
    """A float32 [P] vector of the named kind."""
    rng = np.random.default_rng(seed + 1000 * TOPK_KINDS.index(kind))
    i = np.arange(P, dtype=np.int64)
    sign = (rng.integers(0, 2, P).astype(np.uint32) << 31)
    if kind == "randn":
        return rng.standard_normal(P).astype(np.float32)
    if kind == "equal":
        return np.full(P, 1.5, dtype=np.float32)
    if kind == "sparse":   # P // 5 non-zeros, the rest +0 and -0
        v = sign.copy()
        nz = rng.permutation(P)[:P // 5]
        v[nz] = bits(rng.standard_normal(nz.size).astype(np.float32) + np.float32(3.0))
        return v.view(np.float32)
    if kind == "ties":
        # |v| == 1 on both sides of every chunk boundary and on every sixth coordinate; of the others one in
        # four lies above 1, the rest below: P // 3 falls inside the ties
        mag = (rng.random(P) * 0.9).astype(np.float32)
        big = i % 4 == 1
        mag[big] = np.float32(1.0) + mag[big] + np.float32(0.01)
        tied = (i % 6 == 0) | np.isin(i % CHUNK, (0, 1, CHUNK - 1))
        mag[tied] = np.float32(1.0)
        return (bits(mag) | sign).view(np.float32)
    if kind == "d3":   # one d1, one d2: the last digit decides
        return (np.uint32(0x3F800000) | ((i * 7919) % 512).astype(np.uint32) | sign).view(np.float32)
    if kind == "d2":   # one d1, d3 == 0: the middle digit decides
        return (np.uint32(0x3F800000) | (((i * 7919) % 2048).astype(np.uint32) << 9) | sign).view(np.float32)
    if kind == "extremes":   # denormals beside values near FLT_MAX
        den = rng.integers(1, 0x800000, P).astype(np.uint32)
        top = rng.integers(0x7F000000, 0x7F800000, P).astype(np.uint32)
        return (np.where(i % 3 == 0, top, den).astype(np.uint32) | sign).view(np.float32)
    if kind == "nonfinite":
        v = rng.standard_normal(P).astype(np.float32)
        v[0] = np.nan
        if P >= 4:
            v[P // 2] = np.inf
            v[P - 1] = -np.inf
            v[P // 3] = np.array([0xFFC00001], dtype=np.uint32).view(np.float32)[0]  # a NaN with its sign bit set
        return v
    raise ValueError(kind)


def resolve_k(P: int) -> int:
    return min(P, max(1, int(np.ceil(K_FRACTION * P))))


def round_inputs(K: int, P: int, pad: int, bad: bool = False, seed: int = 0):
    """ROUNDS padded client matrices [K, P + pad] of updates about a common
    base g0: the honest rows share a persistent direction d (what the error
    memory accumulates) under per-round noise whose scale differs from client
    to client (so the update norms spread around any clipping bound); the first
    K // 5 rows are an attacker's, ten times longer, on a direction of its own.  A round's rows
    are base + update; the test adds the round's global model.  bad: row 2 of
    round 0 and row 1 of round 1 are NaN throughout (their beta is 0)."""
    rng = np.random.default_rng(seed + 7 * K + P)
    g0 = rng.standard_normal(P).astype(np.float32)
    d = (0.05 * rng.standard_normal(P)).astype(np.float32)
    evil = (0.05 * rng.standard_normal(P)).astype(np.float32)
    scale = (0.03 + 0.01 * (np.arange(K) % 5)).astype(np.float32)[:, None]
    ups = []
    for t in range(ROUNDS):
        u = d + scale * rng.standard_normal((K, P)).astype(np.float32)
        nmal = K // 5
        u[:nmal] = np.float32(10.0) * evil + (0.01 * rng.standard_normal((nmal, P))).astype(np.float32)
        if bad and t < 2:
            u[2 - t] = np.nan
        ups.append(u.astype(np.float32))
    return g0, ups


def given_clip(K: int, P: int, pad: int, bad: bool = False) -> float:
    """A clip_norm constant between the first round's update norms: half way
    from the lower median of the finite ones to the next larger."""
    g, ups = round_inputs(K, P, pad, bad)
    e = np.sort(norms(g + ups[0], g))
    e = e[np.isfinite(e)]
    m = (e.size - 1) // 2
    return float(0.5 * (e[m] + e[min(m + 1, e.size - 1)]))


def padded(rows: np.ndarray, pad: int) -> np.ndarray:
    K, P = rows.shape
    data = np.full((K, P + pad), FILL, dtype=np.float32)
    data[:, :P] = rows
    return data


def run_rounds(K: int, P: int, pad: int, bad: bool = False, rho: float = 0.0, clip_norm: Optional[float] = None,
               norms_of=norms, k: Optional[int] = None):
    """ROUNDS consecutive calls of the reference on round_inputs: a list of
    (padded matrix, g, Round), each round's g the round before's result.
    norms_of(padded matrix, g) -> float64 [K]: the update norms' source (the
    device's sum order may depend on the row stride, so it sees the layout the
    defense will)."""
    g, ups = round_inputs(K, P, pad, bad)
    ref = SparseFed(resolve_k(P) if k is None else k, clip_norm, rho)
    rounds = []
    for u in ups:
        X = (g + u).astype(np.float32)
        data = padded(X, pad)
        r = ref.step(X, g, norms_of(data, g))
        rounds.append((data, g, r))
        g = r.out
    return rounds
