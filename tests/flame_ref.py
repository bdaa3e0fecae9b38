"""CPU restatement of FLAME as include/flr.h fixes it (flr_flame_select,
flr_add_gaussian, around flr_rows_gram and flr_rows_combine_from), in numpy,
and the data generator of the FLAME tests.

The selection is float64 with every operation rounded on its own (numpy ufuncs
never fuse), only + - * / sqrt: given the same G bits it gives the device's
keep, t*, S, L, beta and sigma bit for bit.  The clustering here is a union-find
over ALL pair distances sorted by level (the device merges the edges of a
minimum spanning tree: another route to the same components).  The Gaussian
draws are the Philox block of tests/fang_ref.py through Box-Muller in float64."""
from collections import namedtuple

import numpy as np

from fang_ref import philox4x32_10
from foolsgold_ref import combine  # noqa: F401  (flr_rows_combine_from's restatement, used as ref.combine)

F32 = np.float32
Selection = namedtuple("Selection", "keep beta sigma S tstar L flags margin dist")


def gram(A, center=None):
    """fp64 [K, K], symmetric bit for bit: the rows (minus center, one fp32
    subtraction) times their transpose."""
    A = np.asarray(A, dtype=F32)
    with np.errstate(all="ignore"):
        if center is not None:
            A = A - np.asarray(center, dtype=F32)[None, :]
        A = A.astype(np.float64)
        G = A @ A.T
    return np.triu(G) + np.triu(G, 1).T


def distances(G):
    """(D float64 [K, K], good bool [K], n float64 [K]): d_ij = 1 - G_ij / (n_i *
    n_j), 1 with a zero norm, NaN (no edge) on the diagonal, for a bad row and
    where the arithmetic gives a NaN."""
    G = np.asarray(G, dtype=np.float64)
    K = G.shape[0]
    diag = np.diag(G).copy()
    good = np.isfinite(diag)
    with np.errstate(all="ignore"):
        n = np.sqrt(diag)
        D = 1.0 - G / (n[:, None] * n[None, :])
    zero = (n == 0.0)
    D = np.where(zero[:, None] | zero[None, :], 1.0, D)
    D[~good, :] = np.nan
    D[:, ~good] = np.nan
    D[np.arange(K), np.arange(K)] = np.nan
    return D, good, n


def default_m(K):
    return K // 2 + 1


def cluster(D, good, m):
    """(keep bool [K], t*, margin): the first component of the threshold graph
    that reaches m good rows, by a union-find over the pair distances level by
    level; t* = +inf and keep all False when there is none; margin = the
    smallest |d - t*| over the pair distances other than t* (inf without)."""
    K = D.shape[0]
    keep = np.zeros(K, dtype=bool)
    if m == 1:
        keep[:] = good
        return keep, (0.0 if good.any() else np.inf), np.inf
    iu, ju = np.triu_indices(K, 1)
    d = D[iu, ju]
    ok = ~np.isnan(d)
    iu, ju, d = iu[ok], ju[ok], d[ok]
    order = np.argsort(d, kind="stable")
    iu, ju, d = iu[order], ju[order], d[order]
    parent = list(range(K))
    size = [1] * K

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    e, E = 0, len(d)
    best, broot, tstar = 0, -1, np.inf
    while e < E:
        w = d[e]
        while e < E and d[e] == w:
            a, c = find(int(iu[e])), find(int(ju[e]))
            e += 1
            if a == c:
                continue
            if size[a] < size[c]:
                a, c = c, a
            parent[c] = a
            size[a] += size[c]
            if size[a] > best:
                best, broot = size[a], a
        if best >= m:
            tstar = float(w)
            break
    if not np.isfinite(tstar) and not (best >= m):
        return keep, np.inf, np.inf
    for i in range(K):
        keep[i] = good[i] and find(i) == broot
    other = d[d != tstar]
    margin = float(np.abs(other - tstar).min()) if other.size else np.inf
    return keep, tstar, margin


def clustering(G, m=None):
    """Steps 1-3 of flr_flame_select: (D, good, n, keep, t*, margin); the input of weights()."""
    G = np.asarray(G, dtype=np.float64)
    K = G.shape[0]
    m = default_m(K) if m is None else m
    assert m <= K < 2 * m
    D, good, n = distances(G)
    return (D, good, n) + cluster(D, good, m)


def select(G, m=None, lam=0.0, norms=None):
    """flr_flame_select on the CPU: a Selection (keep int32 [K], beta float32 [K],
    sigma float32, S, t*, L, flags, the margin of cluster(), the distances)."""
    return weights(clustering(G, m), lam, norms)


def weights(clustered, lam=0.0, norms=None):
    """Step 4 of flr_flame_select on clustering()'s result: a Selection."""
    D, good, n, keep, tstar, margin = clustered
    K = len(n)
    L = int(keep.sum())
    e = n if norms is None else np.asarray(norms, dtype=np.float64)
    S = np.sort(e)[(K - 1) // 2]                      # NaN sorted last
    with np.errstate(all="ignore"):
        gamma = np.where(e > S, S / e, 1.0)
        beta = np.where(keep, gamma / np.float64(L), 0.0).astype(F32) if L else np.zeros(K, dtype=F32)
        sigma = F32(np.float64(lam) * S) if L else F32(0.0)
    flags = (0 if L else 1) | (0 if good.all() else 2)
    return Selection(keep.astype(np.int32), beta, sigma, S, tstar, L, flags, margin, D)


def normals(P, seed=0, stream=0, col0=0):
    """z float64 [P] of flr_add_gaussian, evaluated in float64: the global
    indices 4c .. 4c + 3 share the Philox block with counter (c lo, c hi, 0,
    stream) and key (seed lo, seed hi); Box-Muller on (w0, w1) and (w2, w3)."""
    c0 = col0 >> 2
    nb = ((col0 + P - 1) >> 2) - c0 + 1
    c = np.arange(nb, dtype=np.uint64) + np.uint64(c0)
    lo = np.uint64(0xFFFFFFFF)
    w = philox4x32_10([c & lo, c >> np.uint64(32), np.zeros(nb, dtype=np.uint64), np.full(nb, stream, dtype=np.uint64)],
                      [np.full(nb, seed & 0xFFFFFFFF, dtype=np.uint64),
                       np.full(nb, (seed >> 32) & 0xFFFFFFFF, dtype=np.uint64)])
    z = np.empty((nb, 4))
    for a in (0, 2):
        u1 = ((w[a] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        u2 = (w[a + 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        z[:, a] = r * np.cos(2.0 * np.pi * u2)
        z[:, a + 1] = r * np.sin(2.0 * np.pi * u2)
    off = col0 - 4 * c0
    return z.reshape(-1)[off:off + P]


def add_noise(v, sigma, z):
    """fl(v + fl(sigma * z)) in float32; sigma == 0 returns v's bits."""
    v = np.asarray(v, dtype=F32)
    if F32(sigma) == 0:
        return v.copy()
    with np.errstate(all="ignore"):
        return v + F32(sigma) * np.asarray(z, dtype=F32)


def rounds(K, P, f, nrounds=2, seed=1):
    """(g, [X_1, ..., X_nrounds]): a global model g ~ N(0, 0.05^2) (fp32) and per
    round the clients' models X = fl(g + fl(u)): honest row i >= f: u_i = 0.01 *
    (1 + 0.5 i / K) * (c + 0.8 eps_i); attacker i < f: u_i = 0.05 * (b + 0.05
    eps_i); c and b fixed N(0, 1) directions, eps_i ~ N(0, 1).  Seeded per (K, P).

    What the tests assert of these rows (no attacker admitted, m or m + 1 rows
    admitted) is typical of the rule, not guaranteed by it: over the seeds 0..5
    about one round in fifteen admits m + 2 or m + 3 rows (two small components
    merge at t*), and at (5, 7, 2) one seed in six admits the attackers.  Seed 1
    is a seed at which every shape of the tests is in the typical regime."""
    rng = np.random.default_rng([seed, K, P])
    g = (0.05 * rng.standard_normal(P)).astype(F32)
    c = rng.standard_normal(P)
    b = rng.standard_normal(P)
    scale = 0.01 * (1.0 + 0.5 * np.arange(K) / K)
    out = []
    for _ in range(nrounds):
        eps = rng.standard_normal((K, P))
        U = scale[:, None] * (c[None, :] + 0.8 * eps)
        U[:f] = 0.05 * (b[None, :] + 0.05 * eps[:f])
        out.append(g[None, :] + U.astype(F32))
    return g, out


def row_norms(X, center):
    """float64 [K]: ||x_i - center|| with fp32 differences."""
    U = (np.asarray(X, dtype=F32) - np.asarray(center, dtype=F32)[None, :]).astype(np.float64)
    return np.sqrt((U * U).sum(axis=1))


def run(g, X, m=None, lam=0.0, on="updates"):
    """(noiseless aggregate fp32 [P], Selection) of one call with center g."""
    if on == "updates":
        sel = select(gram(X, g), m, lam)
    else:
        sel = select(gram(X), m, lam, row_norms(X, g))
    return combine(X, g, sel.beta), sel
