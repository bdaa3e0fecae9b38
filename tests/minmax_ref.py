"""Reference of the Min-Max / Min-Sum attacks (flr_minmax_rows, include/flr.h):
numpy / torch on the CPU.  The bit-defined parts restate the header op for op
(mu and sigma through colluding_ref; the perturbation; R2 and S from a given D;
gamma from given statistics in numpy float64; the rows from a given gamma); the
statistics a_i, b_i, c, whose summation order is the kernel's own, are given
here as their accurate values (exact float64 products, math.fsum).  The paper's
halving search is the independent check of the closed form."""
import math

import numpy as np
import torch

from colluding_ref import ALIE, collude

MAX, SUM = 0, 1            # FLR_MINMAX_*
STD, SIGN, UNIT = 0, 1, 2  # FLR_PERTURB_*


def mean_std(X: torch.Tensor, nmal: int):
    """flr_collude_rows' mu and sigma of the benign rows [nmal, K)."""
    _, mu, sigma = collude(X, nmal, ALIE, 0.0)
    return mu, sigma


def perturbation(mu: torch.Tensor, sigma: torch.Tensor, g, perturb: int) -> torch.Tensor:
    """p, fp32: -sigma; -sign(mu - g) with sign(0) = 0 and sign(NaN) = NaN
    (torch.sign gives 0 for NaN, hence the explicit form); -(mu - g)."""
    if perturb == STD:
        return -sigma
    t = mu - g
    if perturb == UNIT:
        return -t
    assert perturb == SIGN
    one = torch.ones_like(t)
    return -torch.where(t > 0, one, torch.where(t < 0, -one, torch.where(t == 0, torch.zeros_like(t), t)))


def statistics(X: torch.Tensor, nmal: int, mu: torch.Tensor, p: torch.Tensor):
    """(a [nb], b [nb], c), the accurate values: d = fl32(mu - x_i), the
    products exact in float64, the sums correctly rounded (math.fsum)."""
    p64 = p.double().numpy()
    a, b = [], []
    for i in range(nmal, X.shape[0]):
        d = (mu - X[i]).double().numpy()
        a.append(math.fsum(d * d))
        b.append(math.fsum(p64 * d))
    return np.array(a), np.array(b), math.fsum(p64 * p64)


def bounds(D: np.ndarray):
    """(R2, S) from the float64 nb x nb distance matrix D, the header's order:
    R2 = max D*D; S = max over the rows of the sequential sum of D*D (cumsum is
    sequential; np.sum is pairwise).  np.max keeps a NaN."""
    D2 = D * D
    return float(np.max(D2)), float(np.max(np.cumsum(D2, axis=1)[:, -1]))


def gamma_closed(a: np.ndarray, b: np.ndarray, c: float, R2: float, S: float, objective: int) -> float:
    """gamma from the statistics, numpy float64, every operation correctly
    rounded, in the header's order: bit-defined."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    c, R2, S = np.float64(c), np.float64(R2), np.float64(S)
    if np.isnan(a).any() or np.isnan(b).any() or np.isnan(c) or np.isnan(R2) or np.isnan(S):
        return float("nan")
    if c == 0.0:
        return 0.0
    if objective == MAX:
        with np.errstate(invalid="ignore"):   # inf - inf: a NaN root, which np.min keeps
            h = np.maximum(R2 - a, 0.0)
            return float(np.min((np.sqrt(b * b + c * h) - b) / c))
    A, Bs = np.cumsum(a)[-1], np.cumsum(b)[-1]   # sequential from 0.0
    h = np.maximum(S - A, 0.0)
    n = np.float64(len(a)) * c
    return float((np.sqrt(Bs * Bs + n * h) - Bs) / n)


def rows(X: torch.Tensor, nmal: int, mu: torch.Tensor, p: torch.Tensor, gamma: float) -> torch.Tensor:
    """A copy of X whose rows [0, nmal) hold fl(mu + fl((float)gamma * p)); a
    NaN gamma leaves them as they were.  Bit-defined."""
    out = X.clone()
    if not math.isnan(gamma):
        out[:nmal] = mu + torch.tensor(np.float32(gamma)) * p
    return out


def true_sq_distances(X: torch.Tensor, nmal: int) -> np.ndarray:
    """The benign rows' squared distances in float64 (no fp32 rounding)."""
    B = X[nmal:].double().numpy()
    return ((B[:, None, :] - B[None, :, :]) ** 2).sum(axis=2)


def attack(X: torch.Tensor, nmal: int, objective: int, perturb: int, g=None, D=None):
    """The whole attack on the CPU with the accurate statistics: (matrix, gamma,
    (a, b, c, R2, S)).  D: the benign rows' float64 distance matrix (None: the
    square roots of true_sq_distances)."""
    mu, sigma = mean_std(X, nmal)
    p = perturbation(mu, sigma, g, perturb)
    a, b, c = statistics(X, nmal, mu, p)
    R2, S = bounds(np.sqrt(true_sq_distances(X, nmal)) if D is None else D)
    gamma = gamma_closed(a, b, c, R2, S, objective)
    return rows(X, nmal, mu, p, gamma), gamma, (a, b, c, R2, S)


def halving_search(X: torch.Tensor, nmal: int, objective: int, mu: torch.Tensor, p: torch.Tensor, gamma_init: float,
                   tau: float = 1e-5):
    """The paper's search (Algorithm 1 of Shejwalkar & Houmansadr): step =
    gamma_init / 2; while |gamma_succ - gamma| > tau: a gamma that satisfies the
    constraint is recorded and raised by step / 2, one that does not is lowered
    by step / 2; step halves.  The constraint is evaluated in float64 on the
    true squared distances, m = mu + gamma * p formed in float64.  Returns
    (gamma_succ, gamma): the paper's result, the largest probe known to
    satisfy the constraint, and the last probe.  The moves are +-s_k, s_k =
    gamma_init / 2^(k+2), and after move k the reach left is s_k: the root lies
    within s_(k-1) of probe k, and gamma_succ = probe - s_(k-1) whenever the loop
    ends, so it ends with s_(k-1) <= tau — the last probe is within tau of the
    root and gamma_succ within 2 tau below it (given the root within gamma_init /
    2 of gamma_init)."""
    B = X[nmal:].double().numpy()
    D2 = true_sq_distances(X, nmal)
    bound = D2.max() if objective == MAX else D2.sum(axis=1).max()
    mu64, p64 = mu.double().numpy(), p.double().numpy()

    def ok(gm):
        d2 = ((mu64 + gm * p64 - B) ** 2).sum(axis=1)
        return (d2.max() if objective == MAX else d2.sum()) <= bound

    gm, step, succ = gamma_init, gamma_init / 2, 0.0
    while abs(succ - gm) > tau:
        if ok(gm):
            succ = gm
            gm = gm + step / 2
        else:
            gm = gm - step / 2
        step = step / 2
    return succ, gm
