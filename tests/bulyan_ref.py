"""Reference for Bulyan (El Mhamdi, Guerraoui, Rouault, ICML 2018) in numpy, the
contract of flr_krum_select_iter and flr_median_window_mean_rows
(include/flr.h).  A helper module, not a test file: the selection re-runs the
oracle's Krum scores on the shrinking set, the window mean is the stable
argsort of the distances to the lower median."""
import numpy as np

from oracle import aggregation as orc

# the iterated-selection shapes (K, f, P) shared by the host and the GPU tests
SELECTION_SHAPES = [(7, 1, 257), (11, 2, 257), (23, 5, 1031), (40, 8, 4099), (128, 25, 2049)]


def sizes(n, f):
    """(theta, beta) of n clients, f of them Byzantine."""
    return n - 2 * f, n - 4 * f


def iter_krum(dist, f, theta):
    """dist: np.float64 [n, n].  (picked in pick order, the first iteration's scores)."""
    alive, picked, first = list(range(dist.shape[0])), [], None
    for it in range(theta):
        nr = len(alive)
        m = min(nr - 1, max(1, nr - f - 2))
        sc = orc.krum_scores(dist[np.ix_(alive, alive)], m)
        first = sc if it == 0 else first
        picked.append(alive.pop(int(np.argsort(np.asarray(sc), kind="stable")[0])))
    return picked, first


def window_ranks(S, beta):
    """The sorted column s and the bool mask of the beta ranks taken per column."""
    s = np.sort(S, axis=0)
    med = s[(s.shape[0] - 1) // 2]
    with np.errstate(invalid="ignore"):
        idx = np.argsort(np.abs(s - med), axis=0, kind="stable")[:beta]
    sel = np.zeros(s.shape, bool)
    np.put_along_axis(sel, idx, True, axis=0)
    return s, sel


def window_mean(S, beta):
    """S: np.float32 [theta, P] -> np.float32 [P].  NaN rule: NaNs sort last;
    the result is NaN when a column holds more than theta - beta of them (one
    would be taken) or its median rank is one."""
    S = np.asarray(S, np.float32)
    theta = S.shape[0]
    s, sel = window_ranks(S, beta)
    acc = np.zeros(s.shape[1], np.float32)
    with np.errstate(invalid="ignore"):
        for r in range(theta):
            acc = np.where(sel[r], (acc + s[r]).astype(np.float32), acc)
        out = (acc / np.float32(beta)).astype(np.float32)
    nnan = np.isnan(S).sum(axis=0)
    bad = (nnan > theta - beta) | ((theta - 1) // 2 >= theta - nnan)
    out[bad] = np.nan
    return out
