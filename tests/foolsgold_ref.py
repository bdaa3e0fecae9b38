"""CPU restatement of FoolsGold as include/flr.h fixes it (flr_rows_accumulate,
flr_rows_gram, flr_foolsgold_weights, flr_rows_combine_from), in numpy, and the
data generator of the FoolsGold tests.  The Gram matrix is numpy's fp64 matrix
product of the fp32 rows (exact products, numpy's summation order); the fp32
passes are numpy float32 operations, each separately rounded."""
from collections import namedtuple

import numpy as np

Weights = namedtuple("Weights", "alpha beta max_cosine flags margin top")


def accumulate(H, X, center):
    """H + (X - center), two fp32 operations per element."""
    H, X, center = (np.asarray(a, dtype=np.float32) for a in (H, X, center))
    with np.errstate(all="ignore"):
        return H + (X - center[None, :])


def gram(A, center=None):
    """fp64 [K, K]: the rows (minus center, one fp32 subtraction) times their transpose."""
    A = np.asarray(A, dtype=np.float32)
    with np.errstate(all="ignore"):
        if center is not None:
            A = A - np.asarray(center, dtype=np.float32)[None, :]
        A = A.astype(np.float64)
        return A @ A.T


def weights(G, kappa=1.0):
    """alpha fp64 [K], beta fp32 [K], max_cosine fp64 [K], flags (bit 0: no
    update, bit 1: a bad row); margin: the distance from 0 of the nearest finite
    pre-clip value kappa * (logit + 0.5) (inf when there is none); top: the
    largest w before the rescaling (-1 with every row bad)."""
    G = np.asarray(G, dtype=np.float64)
    K = G.shape[0]
    d = np.diag(G).copy()
    good = np.isfinite(d)
    with np.errstate(all="ignore"):
        n = np.where(good, np.sqrt(np.where(good, d, 0.0)), 0.0)
        ok = n > 0                                   # false for a NaN norm too
        pair = ok[:, None] & ok[None, :] & ~np.eye(K, dtype=bool)
        cs = np.where(pair, G / (n[:, None] * n[None, :]), 0.0)
        v = np.fmax(cs, 0.0).max(axis=1)             # the diagonal's 0 takes part; a NaN does not
        lower = v[:, None] < v[None, :]
        pc = np.where(lower, cs * v[:, None] / v[None, :], cs)
        mp = np.fmax(pc, 0.0).max(axis=1)
        w = np.minimum(1.0, np.maximum(0.0, 1.0 - mp))
        top = float(w[good].max()) if good.any() else -1.0
        alpha = np.zeros(K)
        margin = float("inf")
        if top > 0.0:
            if K == 1:
                alpha[:] = 1.0
            else:
                wn = np.minimum(w / top, 0.99)
                pre = kappa * (np.log(wn / (1.0 - wn)) + 0.5)
                pre_good = pre[good & np.isfinite(pre)]
                if pre_good.size:
                    margin = float(np.abs(pre_good).min())
                alpha = np.where(good, np.minimum(1.0, np.maximum(0.0, pre)), 0.0)
        v = np.where(good, v, 0.0)
    S = 0.0
    for a in alpha:
        S += float(a)
    beta = (alpha / S).astype(np.float32) if S > 0.0 else np.zeros(K, dtype=np.float32)
    flags = (0 if S > 0.0 else 1) | (0 if good.all() else 2)
    return Weights(alpha, beta, v, flags, margin, top)


def combine(X, center, beta):
    """center + sum_i (x_i - center) * beta_i: fp32, rows ascending, the rows
    with beta_i == 0 skipped."""
    X = np.asarray(X, dtype=np.float32)
    c = np.asarray(center, dtype=np.float32)
    beta = np.asarray(beta, dtype=np.float32)
    acc = np.zeros_like(c)
    with np.errstate(all="ignore"):
        for i in range(X.shape[0]):
            if beta[i] != 0:
                acc = acc + (X[i] - c) * beta[i]
        return c + acc


def rounds(K, P, f, nrounds=3, seed=1):
    """(g, [X_1, ..., X_nrounds]): a global model g = N(0, 1) and per round the
    clients' models g + update (fp32): honest updates 0.01 * (0.45 * c + N(0, 1))
    with one common direction c, the f sybils (rows 0..f-1) 0.01 * (d + 0.1 *
    N(0, 1)) with one common d."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(P).astype(np.float32)
    c = rng.standard_normal(P)
    d = rng.standard_normal(P)
    out = []
    for _ in range(nrounds):
        U = np.empty((K, P))
        U[:f] = 0.01 * (d[None, :] + 0.1 * rng.standard_normal((f, P)))
        U[f:] = 0.01 * (0.45 * c[None, :] + rng.standard_normal((K - f, P)))
        out.append(g[None, :] + U.astype(np.float32))
    return g, out


def run(g, Xs, kappa=1.0, use_memory=True):
    """The defense over successive calls on the rows Xs with the fixed center g:
    a list of (aggregate fp32 [P], Weights, H or None)."""
    H = None
    res = []
    for X in Xs:
        if use_memory:
            H = accumulate(np.zeros_like(X) if H is None else H, X, g)
            G = gram(H)
        else:
            G = gram(X, g)
        wt = weights(G, kappa)
        res.append((combine(X, g, wt.beta), wt, None if H is None else H.copy()))
    return res
