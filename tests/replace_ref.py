"""Reference of model replacement (flr_replace_strength, flr_scale_rows_from;
include/flr.h): numpy on the CPU, the header restated operation for operation.
The strength is float64 with every operation rounded on its own (numpy ufuncs
never fuse), only + - * / sqrt; the scale is three float32 operations.  The
norms and the Gram matrix are inputs: the device tests pass the device's own
(ops.row_norms / ops.rows_gram), the host tests the accurate ones of
norms_gram."""
import numpy as np
import torch

NONE, NORM, DISTANCE = 0, 1, 2  # FLR_REPLACE_* (mode)
MEDIAN, MAX, MEAN = 0, 1, 2     # FLR_REPLACE_* (stat)


def updates(K: int, f: int, P: int, seed: int, amp: float = 1.0):
    """(X float32 [K, P], g float32 [P]): g a random model, the benign updates
    0.1 * d + 0.1 * noise around one common direction d, the attackers' the
    same plus amp * 0.1 * t for one shared backdoor direction t."""
    gen = torch.Generator().manual_seed(1000 * seed + 10 * K + f)
    g = torch.randn(P, generator=gen)
    d = torch.randn(P, generator=gen)
    t = torch.randn(P, generator=gen)
    U = 0.1 * d + 0.1 * torch.randn(K, P, generator=gen)
    U[:f] += amp * 0.1 * t
    return (g + U).contiguous(), g


def centered(X: torch.Tensor, g: torch.Tensor) -> np.ndarray:
    """float64 [K, P] of the float32 differences fl(x - g) (what the norms and
    the Gram matrix are taken of)."""
    return (X - g).double().numpy()


def norms_gram(X: torch.Tensor, g: torch.Tensor):
    """(norms float64 [K], G float64 [K, K] symmetric bit for bit) of the
    centered rows, accurate to float64 rounding."""
    U = centered(X, g)
    G = U @ U.T
    G = np.tril(G) + np.tril(G, -1).T
    return np.sqrt(np.diag(G)).copy(), G


def statistic(e: np.ndarray, stat: int) -> float:
    """B of the benign norms e (float64 [nb]); NaN when one of them is."""
    if np.isnan(e).any():
        return float("nan")
    nb = len(e)
    if stat == MEDIAN:
        s = np.sort(e)
        return float(s[nb // 2]) if nb & 1 else float((s[nb // 2 - 1] + s[nb // 2]) / np.float64(2.0))
    if stat == MAX:
        return float(e.max())
    assert stat == MEAN
    s = np.float64(e[0])
    for v in e[1:]:
        s = s + v
    return float(s / np.float64(nb))


def largest_distance2(G: np.ndarray, f: int) -> float:
    """D2 = max(0, max_{j<k benign} ((G_jj + G_kk) - 2 * G_kj)), a NaN kept."""
    Gb = G[f:, f:]
    d = np.diag(Gb)
    with np.errstate(invalid="ignore"):
        T = (d[None, :] + d[:, None]) - 2.0 * Gb   # [k, j]
    low = T[np.tril_indices(len(d), -1)]
    if np.isnan(low).any():
        return float("nan")
    return float(max(0.0, low.max()))


def strength(norms, G, K: int, f: int, boost: float, mode: int, stat: int = MEDIAN, rho: float = 1.0):
    """(gamma float64 [f], status int32 [f], flags int) as flr_replace_strength."""
    boost, rho = np.float64(boost), np.float64(rho)
    gamma = np.ones(f, dtype=np.float64)
    status = np.full(f, 3, dtype=np.int32)
    if mode == NONE:
        return np.full(f, boost), np.zeros(f, dtype=np.int32), 0
    if mode == NORM:
        B = statistic(np.asarray(norms[f:], dtype=np.float64), stat)
    else:
        B = largest_distance2(G, f)
    if not np.isfinite(B):
        return gamma, status, 1
    B = np.float64(B)
    flags = 0
    with np.errstate(all="ignore"):
        for i in range(f):
            own = np.float64(norms[i]) if mode == NORM else np.float64(G[i, i])
            bad = not np.isfinite(own) or (mode == DISTANCE and norms is not None and not np.isfinite(norms[i]))
            if bad:
                flags |= 2
                continue
            if own == 0.0:
                gamma[i], status[i] = boost, 0
                continue
            if mode == NORM:
                bound = rho * B
                if boost * own <= bound:
                    gamma[i], status[i] = boost, 0
                else:
                    gamma[i], status[i] = bound / own, 1
                continue
            b2 = (rho * rho) * B
            a = own
            b = G[f:, i]                       # G_ji for G_ij, as the kernel
            c = np.diag(G)[f:] - b2
            disc = b * b - a * c
            infeasible = bool((disc < 0.0).any())
            disc = np.where(disc < 0.0, 0.0, disc)
            roots = (b + np.sqrt(disc)) / a
            m = np.float64("nan") if np.isnan(roots).any() else roots.min()
            if m != m:
                flags |= 2
                continue
            if m < 0.0:
                infeasible, m = True, np.float64(0.0)
            gi = m if m < boost else boost
            gamma[i] = gi
            status[i] = 2 if infeasible else (1 if gi < boost else 0)
    return gamma, status, flags


def scale(X: torch.Tensor, g: torch.Tensor, gamma32, n: int = None) -> torch.Tensor:
    """flr_scale_rows_from on the CPU: a copy of X with rows i < n replaced by
    fl(g + fl(fl(x - g) * gamma_i)), float32; gamma_i == 1 or NaN keeps the row."""
    gam = np.asarray(gamma32, dtype=np.float32)
    n = len(gam) if n is None else n
    out = X.clone()
    c = g.numpy().astype(np.float32, copy=False)
    with np.errstate(all="ignore"):
        for i in range(n):
            gi = gam[i]
            if gi == np.float32(1.0) or gi != gi:
                continue
            x = X[i].numpy()
            r = c + (x - c) * gi
            assert r.dtype == np.float32
            out[i] = torch.from_numpy(r)
    return out


def worst_distance2(U: np.ndarray, f: int, i: int, gamma: float) -> float:
    """max_j ||gamma u_i - u_j||^2 over the benign rows, evaluated directly."""
    D = gamma * U[i][None, :] - U[f:]
    return float((D * D).sum(axis=1).max())


def diameter2(U: np.ndarray, f: int) -> float:
    """max_{j,k benign} ||u_j - u_k||^2, evaluated directly."""
    Ub = U[f:]
    best = 0.0
    for j in range(len(Ub)):
        D = Ub[j][None, :] - Ub[j + 1:]
        if len(D):
            best = max(best, float((D * D).sum(axis=1).max()))
    return best
