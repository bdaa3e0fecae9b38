"""Reference of centered clipping (flr_centered_clip, include/flr.h): the
header's arithmetic restated on the CPU.  Distances in numpy float64 from fp32
differences; scales in numpy float32 (each op one IEEE-rounded fp32 operation);
the step as a row loop of torch fp32 ops, each rounded on its own, so the kernel
has to match out, the scales and the thresholds bit for bit.

The kernel's distances are summed in another order than numpy's, so they agree
to ~1e-15 relative, not bit for bit, and the scales start from (float)d.  The
reference therefore also returns a margin: how close, relatively, any distance
it computed came to a point where that last-bits difference could change a
float32 — the midpoint of two adjacent float32 values.  (In fixed-tau mode it
also takes the relative gap between d32 and tau where they differ, the distance
of the comparison's operands.)  A test asserts the margin is far above the
summation error before it compares the scales bit for bit."""
import numpy as np
import torch


def _midpoint_gap(d: np.ndarray) -> float:
    """Smallest relative gap between a finite, non-zero float64 distance and the
    nearest midpoint of two adjacent float32 values."""
    d = d[np.isfinite(d) & (d != 0)]
    d32 = d.astype(np.float32)
    d = d[np.isfinite(d32)]
    d32 = d32[np.isfinite(d32)]
    if d.size == 0:
        return float("inf")
    up = np.nextafter(d32, np.float32(np.inf)).astype(np.float64)
    dn = np.nextafter(d32, np.float32(-np.inf)).astype(np.float64)
    c = d32.astype(np.float64)
    gap = np.minimum(np.abs(d - 0.5 * (c + up)), np.abs(d - 0.5 * (c + dn)))
    return float(np.min(gap / np.abs(d)))


def distances(X: torch.Tensor, v: torch.Tensor) -> np.ndarray:
    """float64 [K]: ||x_i - v||, fp32 differences, float64 squares and sum."""
    diff = (X - v).numpy().astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt((diff * diff).sum(axis=1))


def scales(d: np.ndarray, tau: float):
    """(s float32 [K], t float32): the header's scale rule on float32(d)."""
    with np.errstate(over="ignore"):
        d32 = d.astype(np.float32)
    K = d32.shape[0]
    t = np.float32(tau) if tau > 0 else np.sort(d32)[(K - 1) // 2]   # numpy sorts NaN last
    s = np.ones(K, dtype=np.float32)
    with np.errstate(invalid="ignore", divide="ignore", under="ignore"):
        clip = d32 > t
        s[clip] = t / d32[clip]          # float32 / float32: one correctly rounded division
    s[np.isnan(d32)] = np.float32(0)
    return s, t


def step(X: torch.Tensor, v: torch.Tensor, s: np.ndarray) -> torch.Tensor:
    """v' = v + (sum over the rows with s_i != 0, in order, of (x_i - v) * s_i) / K."""
    K, P = X.shape
    acc = torch.zeros(P, dtype=torch.float32)
    for i in range(K):
        if s[i] != 0:
            acc = acc + (X[i] - v) * torch.tensor(float(s[i]), dtype=torch.float32)
    return v + acc / torch.tensor(float(K), dtype=torch.float32)


def centered_clip(X: torch.Tensor, v0: torch.Tensor, tau: float, iters: int):
    """X: CPU float32 [K, P], v0: CPU float32 [P]; tau = 0: median mode.
    Returns (out float32 [P], norms float64 ndarray [iters, K], scales float32
    tensor [iters, K], taus float32 tensor [iters], margin float)."""
    assert X.dtype == torch.float32 and X.device.type == "cpu" and X.dim() == 2
    assert v0.dtype == torch.float32 and v0.shape == (X.shape[1],)
    assert iters >= 1 and tau >= 0
    K = X.shape[0]
    norms = np.empty((iters, K), dtype=np.float64)
    sc = np.empty((iters, K), dtype=np.float32)
    taus = np.empty(iters, dtype=np.float32)
    margin = float("inf")
    v = v0.clone()
    for l in range(iters):
        d = distances(X, v)
        s, t = scales(d, tau)
        norms[l], sc[l], taus[l] = d, s, t
        margin = min(margin, _midpoint_gap(d))
        if tau > 0:
            with np.errstate(over="ignore"):
                d32 = d.astype(np.float32)
            d32 = d32[np.isfinite(d32) & (d32 != np.float32(tau))].astype(np.float64)
            if d32.size:
                margin = min(margin, float(np.min(np.abs(d32 - np.float64(np.float32(tau))))
                                           / np.float64(np.float32(tau))))
        v = step(X, v, s)
    return v, norms, torch.from_numpy(sc), torch.from_numpy(taus), margin
