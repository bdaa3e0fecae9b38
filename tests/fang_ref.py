"""Reference of Fang et al.'s attacks (flr_fang_krum_strength, flr_fang_krum_rows,
flr_fang_trim_rows; include/flr.h): numpy on the CPU, the header restated
operation for operation.  The strength is float64 with every operation rounded
on its own (numpy ufuncs never fuse), only + - * / sqrt; the rows are float32.
G, b and c are inputs: the device tests pass the device's own, the host tests
the accurate ones of statistics()."""
import numpy as np
import torch

F32 = np.float32


def mean_sign(X: torch.Tensor, g: torch.Tensor, f: int):
    """(mu float32 [P], s float32 [P]): the benign rows' mean as
    flr_collude_rows forms it (sequential float32 adds from 0, one division) and
    s = sign(fl(mu - g)), sign(0) = 0, sign(NaN) = NaN."""
    Xb = X[f:].numpy()
    acc = np.zeros(Xb.shape[1], dtype=F32)
    with np.errstate(all="ignore"):
        for row in Xb:
            acc = acc + row
        mu = acc / F32(len(Xb))
        t = mu - g.numpy()
        s = np.where(t > 0, F32(1), np.where(t < 0, F32(-1), np.where(t == 0, F32(0), t))).astype(F32)
    assert mu.dtype == F32 and t.dtype == F32
    return mu, s


def statistics(X: torch.Tensor, g: torch.Tensor, f: int):
    """(G float64 [nb, nb] symmetric bit for bit, b float64 [nb], c float) of the
    benign rows about g, accurate to float64 rounding."""
    _, s = mean_sign(X, g, f)
    U = (X[f:] - g).double().numpy()
    G = U @ U.T
    G = np.tril(G) + np.tril(G, -1).T
    sd = s.astype(np.float64)
    return G, U @ sd, float(sd @ sd)


def _seq_sum(v) -> np.ndarray:
    """The sequential float64 sum from 0.0 along the last axis (numpy's cumsum
    adds one element after the other)."""
    v = np.asarray(v, dtype=np.float64)
    zero = np.zeros(v.shape[:-1] + (1,))
    return np.cumsum(np.concatenate([zero, v], axis=-1), axis=-1)[..., -1]


def _nan_min(v) -> np.float64:
    v = np.asarray(v, dtype=np.float64)
    return np.float64("nan") if np.isnan(v).any() else v.min()


def sorted_rows(G: np.ndarray) -> np.ndarray:
    """r float64 [nb, nb - 1]: row i's distances to the others, ascending, NaN last."""
    nb = G.shape[0]
    e = np.diag(G)
    with np.errstate(invalid="ignore"):
        x = (e[:, None] + e[None, :]) - 2.0 * G
        D = np.sqrt(np.where(x < 0.0, 0.0, x))
    return np.stack([np.sort(np.delete(D[i], i)) for i in range(nb)])


def probe(r: np.ndarray, e, b, c, K: int, f: int, lam):
    """(S_att, S_min) of one lambda."""
    m, na = K - f - 2, K - 2 * f - 1
    lam = np.float64(lam)
    with np.errstate(all="ignore"):
        x = (e + (2.0 * lam) * b) + (lam * lam) * c
        d = np.sqrt(np.where(x < 0.0, 0.0, x))
        satt = _seq_sum(np.sort(d)[:na])
        S = _seq_sum(np.sort(np.concatenate([r, np.repeat(d[:, None], f, axis=1)], axis=1), axis=1)[:, :m])
    return satt, _nan_min(S)


def strength(G, b, c, K: int, f: int, threshold: float = 1e-5):
    """(lambda float64, status, t, stats float64 [5]: lambda0, T, E, the last
    probe's S_att and S_min) as flr_fang_krum_strength."""
    nan = np.float64("nan")
    G = np.asarray(G, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    c = np.float64(c)
    threshold = np.float64(threshold)
    m, na = K - f - 2, K - 2 * f - 1
    assert G.shape == (K - f, K - f) and K >= 2 * f + 3 and f >= 1
    e = np.diag(G).copy()
    r = sorted_rows(G)
    with np.errstate(all="ignore"):
        T = _nan_min(_seq_sum(r[:, :m]))
        E = np.float64("nan") if np.isnan(e).any() else np.sqrt(e).max()
        stats = np.array([nan, T, E, nan, nan])
        if np.isnan(e).any() or np.isnan(b).any() or np.isnan(c) or np.isnan(T):
            return nan, 3, 0, stats
        if c == 0.0:
            return np.float64(0.0), 2, 0, stats
        rc = np.sqrt(c)
        lam0 = T / (np.float64(na) * rc) + E / rc
        stats[0] = lam0
        if not np.isfinite(lam0):
            return nan, 3, 0, stats
        lam, t = lam0, 0
        while True:
            if lam <= threshold:
                return lam, 1, t, stats
            stats[3], stats[4] = probe(r, e, b, c, K, f, lam)
            if stats[3] <= stats[4]:
                return lam, 0, t, stats
            lam = lam * np.float64(0.5)
            t += 1


def krum_rows(X: torch.Tensor, g: torch.Tensor, f: int, lam32) -> torch.Tensor:
    """flr_fang_krum_rows' last stage on the CPU: a copy of X with rows i < f
    replaced by fl(g - fl(lambda32 * s)), float32; a NaN lambda keeps the rows."""
    out = X.clone()
    lam32 = F32(lam32)
    if lam32 != lam32:
        return out
    _, s = mean_sign(X, g, f)
    with np.errstate(all="ignore"):
        row = g.numpy() - lam32 * s
    assert row.dtype == F32
    out[:f] = torch.from_numpy(row)
    return out


def krum_pick(X: torch.Tensor, f: int) -> int:
    """Krum's pick over the rows of X evaluated directly in float64: the score is
    the sum of the K - f - 2 smallest distances to the others, ties to the lower
    index."""
    Y = X.double().numpy()
    K = len(Y)
    D = np.stack([np.sqrt(((Y[i][None, :] - Y) ** 2).sum(axis=1)) for i in range(K)])
    m = K - f - 2
    scores = np.array([np.sort(np.delete(D[i], i))[:m].sum() for i in range(K)])
    return int(np.argsort(scores, kind="stable")[0])


M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Philox4x32-10 on arrays: ctr four and key two uint32 arrays (or ints) of
    one shape; the four output words."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in ctr]
    k = [np.asarray(v, dtype=np.uint64) & MASK for v in key]
    for r in range(10):
        if r:
            k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
    return [v.astype(np.uint32) for v in c]


def uniforms(P: int, f: int, seed: int, stream: int, col0: int = 0) -> np.ndarray:
    """u float32 [f, P] of flr_fang_trim_rows: (word 0 >> 8) * 2^-24."""
    col = np.broadcast_to(np.arange(col0, col0 + P, dtype=np.uint64)[None, :], (f, P))
    row = np.broadcast_to(np.arange(f, dtype=np.uint64)[:, None], (f, P))
    w = philox4x32_10([col & MASK, col >> np.uint64(32), row, np.full((f, P), stream, dtype=np.uint64)],
                      [np.full((f, P), seed & 0xFFFFFFFF, dtype=np.uint64),
                       np.full((f, P), (seed >> 32) & 0xFFFFFFFF, dtype=np.uint64)])[0]
    return (w >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)


def trim_bounds(X: torch.Tensor, g: torch.Tensor, f: int, b: float):
    """(mu, s, near, far) float32 [P] of flr_fang_trim_rows; near / far are
    meaningless where s is 0 or NaN."""
    mu, s = mean_sign(X, g, f)
    Xb = X[f:].numpy()
    b = F32(b)
    mn, mx = Xb[0].copy(), Xb[0].copy()
    with np.errstate(all="ignore"):
        for row in Xb[1:]:
            mn = np.where(row < mn, row, mn)
            mx = np.where(row > mx, row, mx)
        near = np.where(s > 0, mn, mx)
        far = np.where(s > 0, np.where(mn > 0, mn / b, mn * b), np.where(mx > 0, mx * b, mx / b))
    assert near.dtype == F32 and far.dtype == F32
    return mu, s, near, far


def trim_rows(X: torch.Tensor, g: torch.Tensor, f: int, b: float = 2.0, seed: int = 0, stream: int = 0,
              col0: int = 0) -> torch.Tensor:
    """flr_fang_trim_rows on the CPU: a copy of X with rows i < f replaced."""
    mu, s, near, far = trim_bounds(X, g, f, b)
    u = uniforms(X.shape[1], f, seed, stream, col0)
    with np.errstate(all="ignore"):
        drawn = near[None, :] + u * (far - near)[None, :]
        t = mu - g.numpy()
        rows = np.where((s > 0) | (s < 0), drawn, np.where(s == 0, mu, t)[None, :])
    assert rows.dtype == F32
    out = X.clone()
    out[:f] = torch.from_numpy(np.ascontiguousarray(rows))
    return out
