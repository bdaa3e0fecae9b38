"""Reference of the divide-and-conquer defense (flr_dnc_select and
flr_rows_mean_keep, include/flr.h): the header's arithmetic restated on the CPU.
The column hash in Python ints (mod 2^64); the centering in torch fp32, one
IEEE-rounded op per step, the rows added in order; the Gram matrix and the power
iteration in numpy fp64.  The columns, the kept set, the count and the flag have
to match the kernel exactly, the mean bit for bit; the scores differ from the
kernel's only by the order of the fp64 sums."""
import math

import numpy as np
import torch

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def mix(z: int) -> int:
    """The splitmix64 finaliser."""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def columns(P: int, b: int, seed: int, it: int) -> np.ndarray:
    """Iteration it's b columns: one per stratum [floor(j*P/b), floor((j+1)*P/b))."""
    assert 1 <= b <= P
    out = np.empty(b, dtype=np.int64)
    for j in range(b):
        lo, hi = (j * P) // b, ((j + 1) * P) // b
        h = mix((seed + GOLDEN * (it * b + j + 1)) & M64)
        out[j] = lo + h % (hi - lo)
    return out


def center(S: torch.Tensor):
    """S: the sampled values, fp32 [K, b].  Returns (C fp32 [K, b], bad bool [K])."""
    K = S.shape[0]
    bad = ~torch.isfinite(S).all(dim=1)
    s = torch.zeros(S.shape[1], dtype=torch.float32)
    for i in range(K):
        if not bad[i]:
            s = s + S[i]
    mu = s / torch.tensor(float(int((~bad).sum())), dtype=torch.float32)
    C = torch.zeros_like(S)
    for i in range(K):
        if not bad[i]:
            C[i] = S[i] - mu
    return C, bad


def scores_of(C: torch.Tensor, bad: torch.Tensor, power_iters: int) -> np.ndarray:
    """The squared projections on the top singular direction through the Gram
    matrix; +inf in the bad rows; zeros in the degenerate cases."""
    Cd = C.double().numpy()
    G = Cd @ Cd.T
    K = G.shape[0]
    sc = np.zeros(K)
    d = np.diag(G)
    a = int(np.argmax(d))  # the first of the largest
    if d[a] != 0:
        u = G[:, a] / math.sqrt(float((G[:, a] * G[:, a]).sum()))
        ok = True
        for _ in range(power_iters):
            w = G @ u
            n = math.sqrt(float((w * w).sum()))
            if n == 0:
                ok = False
                break
            u = w / n
        if ok:
            w = G @ u
            lam = float(u @ w)
            if not lam <= 0:
                sc = w * w / lam
    sc = np.array(sc, dtype=np.float64)
    sc[bad.numpy()] = np.inf
    return sc


def keep_of(sc: np.ndarray, bad: np.ndarray, nremove: int):
    """(keep bool [K], gap): ranks ascending by (bad, score, index); the good rows
    of rank < K - nremove; gap between the last kept and the first removed score
    (inf when nothing finite is removed)."""
    K = len(sc)
    order = sorted(range(K), key=lambda i: (bool(bad[i]), sc[i], i))
    keep = np.zeros(K, dtype=bool)
    for r, i in enumerate(order):
        keep[i] = (not bad[i]) and r < K - nremove
    gap = math.inf
    cut = K - nremove
    if 0 < cut < K and not bad[order[cut]] and not bad[order[cut - 1]]:
        gap = float(sc[order[cut]] - sc[order[cut - 1]])
    return keep, gap


def dnc_select(X: torch.Tensor, b: int, niters: int, nremove: int, power_iters: int, seed: int = 0, cols=None):
    """X: CPU float32 [K, P].  Returns (cols int64 [niters, b], scores float64
    [niters, K], keep int32 [K], count, flag, margin): margin is the smallest gap
    between the last kept and the first removed score relative to the largest
    finite score, over the iterations (inf where every score is 0)."""
    assert X.dtype == torch.float32 and X.device.type == "cpu" and X.dim() == 2
    K, P = X.shape
    assert 1 <= b <= P and niters >= 1 and power_iters >= 1 and 0 <= nremove <= K - 1
    used = np.empty((niters, b), dtype=np.int64)
    scores = np.empty((niters, K))
    keeps = []
    margin = math.inf
    for it in range(niters):
        c = columns(P, b, seed, it) if cols is None else np.clip(np.asarray(cols[it], dtype=np.int64), 0, P - 1)
        used[it] = c
        C, bad = center(X[:, torch.from_numpy(c)].contiguous())
        sc = scores_of(C, bad, power_iters)
        keep, gap = keep_of(sc, bad.numpy(), nremove)
        fin = sc[np.isfinite(sc)]
        top = float(fin.max()) if fin.size else 0.0
        if top > 0:
            margin = min(margin, gap / top)
        scores[it] = sc
        keeps.append(keep)
    both = np.logical_and.reduce(keeps)
    flag = 0
    if not both.any():
        both, flag = keeps[0], 1
    return used, scores, torch.from_numpy(both.astype(np.int32)), int(both.sum()), flag, margin


def rows_mean_keep(X: torch.Tensor, keep) -> torch.Tensor:
    """The kept rows' mean: sequential fp32 adds from +0, one division by the
    count (0 / 0 = NaN when nothing is kept)."""
    acc = torch.zeros(X.shape[1], dtype=torch.float32)
    n = 0
    for i in range(X.shape[0]):
        if keep[i]:
            acc = acc + X[i]
            n += 1
    return acc / torch.tensor(float(n), dtype=torch.float32)


def dnc(X: torch.Tensor, b: int, niters: int, nremove: int, power_iters: int, seed: int = 0):
    """The whole rule: (aggregate, keep, margin)."""
    _, _, keep, _, _, margin = dnc_select(X, b, niters, nremove, power_iters, seed)
    return rows_mean_keep(X, keep), keep, margin


def alie_rows(K: int, P: int, f: int, seed: int, z: float = 1.0) -> torch.Tensor:
    """Benign rows g + 0.05 randn; rows [0, f) the ALIE vector mu - z * sigma of
    the benign rows (tests/colluding_ref.py)."""
    from colluding_ref import ALIE, collude
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(P, generator=gen)
    X = g + 0.05 * torch.randn(K, P, generator=gen)
    if f > 0:
        X = collude(X, f, ALIE, z)[0]
    return X.contiguous()
