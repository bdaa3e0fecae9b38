"""Workload generators for the attacked configurations.

* sign flip — InnerProductManipulationAttack.poison_update with no benign
  mean negates the submitted update (src/attacks/model_poisoning.py:274-276),
  applied after local training (malicious_client.py:103-115).  The engine
  negates the malicious rows of the client matrix in place.
* backdoor — BackdoorAttack.poison_data (src/attacks/backdoor.py:115-290):
  a trigger_size x trigger_size square of trigger_value at the bottom-right
  position (h - size - 1, w - size - 1) on every channel of the (normalised)
  image, on poison_ratio of the client's samples chosen with
  np.random.seed(seed) + np.random.choice(range(n), n*ratio, replace=False),
  and the label replaced by target_class (BackdoorDataset, :13-60).
  Applied here to a malicious client's resident synthetic batches before the
  round (data generation, not timed).
* ALIE — "A Little Is Enough" (Baruch, Baruch, Goldberg, NeurIPS 2019): the
  f colluding attackers know the benign updates and all submit mu - z * sigma
  per coordinate (the benign mean and population standard deviation), z from
  the normal quantile that keeps them inside the benign spread (alie_z).  Not
  in the reference; the attack Krum, the trimmed mean and Bulyan are judged by.
* IPM with a benign mean — "Fall of Empires" (Xie, Koyejo, Gupta, UAI 2019),
  the other branch of InnerProductManipulationAttack.poison_update
  (src/attacks/model_poisoning.py, next to the sign flip's -param): every
  attacker submits -epsilon * mu.
  Both are one pass of flr_collude_rows over the exchanged client matrix
  (attackers = rows 0..f-1, overwritten in place), applied by the engine
  between the exchange and the defense.
* Min-Max / Min-Sum — "Manipulating the Byzantine" (Shejwalkar, Houmansadr,
  NDSS 2021): every attacker submits mu + gamma * p, p a perturbation direction
  (-sigma, -sign(mu - g) or -(mu - g)), gamma the largest strength that keeps
  the vector no further from the benign rows than they are from each other
  (the maximum distance, or the sum of squared distances).  Aggregator-
  agnostic, the strength computed from the round's own matrix instead of
  guessed per defense; not in the reference.  One flr_minmax_rows call in the
  same slot (min_max_, min_sum_); it needs whole rows.
* model replacement — "How To Backdoor Federated Learning" (Bagdasaryan et al.,
  AISTATS 2020): the backdoor above, boosted.  The attackers train on the
  triggered data and then submit g + gamma_i * (x_i - g), gamma_i = boost
  (default K / f, the paper's n / eta at server rate 1 shared by the f
  attackers) or what is left of it under the server's bound: rho times a
  statistic of the benign rows' norms (Sun et al. 2019), or rho times the
  benign rows' largest mutual distance (the Min-Max criterion on each
  attacker's own direction).  Not in the reference; what norm_bounding,
  gradient_clipping, dp_sgd, robust_lr, foolsgold and krum are judged by.
  flr_replace_strength + flr_scale_rows_from in the colluding attacks' slot
  (model_replacement_).
* Fang et al.'s attacks — "Local Model Poisoning Attacks to Byzantine-Robust
  Federated Learning" (Fang, Cao, Jia, Gong, USENIX Security 2020): the two
  full-knowledge attacks written against one rule each, the baseline Min-Max
  and Min-Sum measure themselves against; not in the reference.  Both push
  against s = sign(mu - g), the direction the benign clients moved in.
  fang_krum_: every attacker submits g - lambda * s, lambda the largest
  lambda0 * 2^-t for which Krum picks an attacker — what krum and multi_krum
  are judged by; the paper's Krum per probe is closed here into one Gram
  matrix and one statistics pass (flr_fang_krum_rows); it needs whole rows.
  fang_trim_: per coordinate the attackers sit just beyond the benign extreme
  on the side opposite s, at points drawn per attacker — the worst case of
  trimmed_mean, median, Bulyan's second stage and robust_lr round them; one
  coordinate-wise pass (flr_fang_trim_rows) with a counter-based generator
  keyed by the coordinate's index, so it runs on a rank's all-to-all slice.
"""
from __future__ import annotations

import statistics
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops


def sign_flip_(X: torch.Tensor, rows: Sequence[int]) -> None:
    """In place: X[r] = -X[r] for the malicious rows."""
    for r in rows:
        X[r].neg_()


def alie_z(n: int, f: int) -> float:
    """ALIE's z for n clients of which f collude: s = n // 2 + 1 - f benign
    clients must sit farther from the mean than the attackers for them to be in
    the majority, so z = Phi^-1((n - s) / n) (the paper's z_max)."""
    n, f = int(n), int(f)
    s = n // 2 + 1 - f
    if f < 1 or not 1 <= s <= n - 1:
        raise ValueError(f"alie_z needs 1 <= f and 1 <= n // 2 + 1 - f <= n - 1 (got n = {n}, f = {f})")
    return statistics.NormalDist().inv_cdf((n - s) / n)


def _attacked_matrix(X, f: int) -> torch.Tensor:
    """The [K, P] view of a ClientMatrix (or the tensor itself), f checked."""
    M = X if isinstance(X, torch.Tensor) else X.X
    if not 1 <= f < M.shape[0]:
        raise ValueError(f"a colluding attack needs 1 <= f < K (got f = {f}, K = {M.shape[0]})")
    return M


def alie_(X, f: int, z: Optional[float] = None) -> None:
    """In place on a float32 device matrix or a ClientMatrix: rows 0..f-1 <-
    mu - z * sigma of rows f..K-1 (z None: alie_z(K, f))."""
    M = _attacked_matrix(X, f)
    ops.collude_rows(M, f, ops.COLLUDE_ALIE, alie_z(M.shape[0], f) if z is None else z)


def ipm_(X, f: int, epsilon: float = 0.5) -> None:
    """In place on a float32 device matrix or a ClientMatrix: rows 0..f-1 <-
    -epsilon * mu, mu the mean of rows f..K-1."""
    ops.collude_rows(_attacked_matrix(X, f), f, ops.COLLUDE_IPM, epsilon)


PERTURBATIONS = {"std": ops.PERTURB_STD, "sign": ops.PERTURB_SIGN, "unit": ops.PERTURB_UNIT}


def _minmax(X, f: int, objective: int, perturb: str, global_flat) -> torch.Tensor:
    M = _attacked_matrix(X, f)
    if perturb not in PERTURBATIONS:
        raise ValueError(f"unknown perturbation {perturb!r} (one of {', '.join(PERTURBATIONS)})")
    if perturb != "std" and global_flat is None:
        raise ValueError(f"perturbation {perturb!r} needs global_flat, the model the clients started from")
    return ops.minmax_rows(M, f, objective, PERTURBATIONS[perturb], global_flat)


def min_max_(X, f: int, perturb: str = "std", global_flat: Optional[torch.Tensor] = None) -> torch.Tensor:
    """In place on a float32 device matrix or a ClientMatrix: rows 0..f-1 <-
    mu + gamma * p, gamma the largest strength with max_i ||m - x_i|| no larger
    than the largest distance between two benign rows f..K-1.  perturb: "std"
    (p = -sigma), "sign" (p = -sign(mu - g)) or "unit" (p = -(mu - g), not
    normalised; gamma * ||p|| is the paper's unit-vector gamma), g =
    global_flat.  Returns gamma, a float64 device scalar (NaN: a benign row
    held a NaN and the rows were left as they were) — unlike alie_ / ipm_ the
    strength is a result here."""
    return _minmax(X, f, ops.MINMAX_MAX, perturb, global_flat)


def min_sum_(X, f: int, perturb: str = "std", global_flat: Optional[torch.Tensor] = None) -> torch.Tensor:
    """As min_max_, gamma the largest strength with sum_i ||m - x_i||^2 no
    larger than the largest sum of squared distances from one benign row to the
    others."""
    return _minmax(X, f, ops.MINMAX_SUM, perturb, global_flat)


STEALTH = {"none": ops.REPLACE_NONE, "norm": ops.REPLACE_NORM, "distance": ops.REPLACE_DISTANCE}
STATS = {"median": ops.REPLACE_MEDIAN, "max": ops.REPLACE_MAX, "mean": ops.REPLACE_MEAN}


def replacement_config(K: int, f: int, boost=None, stealth: str = "none", stat: str = "median",
                       rho=1.0) -> Tuple[float, int, int, float]:
    """(boost, mode, stat, rho) of model_replacement_ checked on the host: the
    names known, boost (None: K / f) and rho finite numbers > 0, 1 <= f < K, and
    two benign rows for the distance bound."""
    if stealth not in STEALTH:
        raise ValueError(f"unknown stealth {stealth!r} (one of {', '.join(STEALTH)})")
    if stat not in STATS:
        raise ValueError(f"unknown stat {stat!r} (one of {', '.join(STATS)})")
    if not 1 <= f < K:
        raise ValueError(f"model replacement needs 1 <= f < K (got f = {f}, K = {K})")
    if stealth == "distance" and K - f < 2:
        raise ValueError(f"stealth 'distance' needs two benign rows (got K - f = {K - f})")
    boost = K / f if boost is None else ops._positive_finite(boost, "boost")
    return boost, STEALTH[stealth], STATS[stat], ops._positive_finite(rho, "rho")


def replace_rows_(M: torch.Tensor, f: int, g: torch.Tensor, boost: float, mode: int, stat: int, rho: float):
    """model_replacement_ on a matrix with replacement_config's checked values
    (the round engine's call): the statistic pass its mode needs, the strengths,
    the scale; (gamma, status, flags)."""
    norms = ops.row_norms(M, center=g) if mode == ops.REPLACE_NORM else None
    G = ops.rows_gram(M, center=g) if mode == ops.REPLACE_DISTANCE else None
    gamma, gamma32, status, flags = ops.replace_strength(norms, G, f, boost, mode, stat, rho, K=M.shape[0],
                                                         device=M.device)
    ops.scale_rows_from(M, g, gamma32)
    return gamma, status, flags


def model_replacement_(X, f: int, global_flat: torch.Tensor, boost: Optional[float] = None, stealth: str = "none",
                       stat: str = "median", rho: float = 1.0):
    """In place on a float32 device matrix or a ClientMatrix whose rows 0..f-1
    were trained on the backdoor's data: row i <- g + gamma_i * (x_i - g), g =
    global_flat, the model the round trained from.  gamma_i = boost (None: K /
    f) under stealth "none"; "norm": min(boost, rho * B / ||x_i - g||), B the
    stat ("median", "max" or "mean") of the benign rows' ||x_j - g||;
    "distance": the largest gamma_i <= boost that keeps the row within rho
    times the benign rows' largest mutual distance of every benign row.  The
    strengths are solved on the device from the matrix itself: no host round
    trip.  Returns (gamma float64 [f], status int32 [f] — 0 boost-limited, 1
    bound-limited, 2 infeasible (the closest point), 3 left alone —, flags
    int32 [1]: bit 0 a non-finite benign statistic (every row left alone), bit
    1 a non-finite attacker) as device tensors."""
    M = X if isinstance(X, torch.Tensor) else X.X
    return replace_rows_(M, int(f), global_flat, *replacement_config(M.shape[0], int(f), boost, stealth, stat, rho))


def fang_krum_config(K: int, f: int, threshold=ops.FANG_THRESHOLD) -> float:
    """fang_krum_'s threshold checked on the host with the shape: a finite
    number > 0, f >= 1, Krum's own K >= 2f + 3, at most 1024 benign rows."""
    return ops._fang_krum_shape(K, f, threshold)[2]


def fang_krum_(X, f: int, global_flat: torch.Tensor, threshold: float = ops.FANG_THRESHOLD):
    """Fang et al.'s Krum attack, in place on a float32 device matrix or a
    ClientMatrix: rows 0..f-1 <- g - lambda * s, g = global_flat (the model the
    round trained from), s = sign(mu - g) with sign(0) = 0, mu the mean of rows
    f..K-1, lambda the largest lambda0 * 2^-t above threshold for which Krum with
    num_malicious = f picks one of those rows (lambda0 the paper's upper bound).
    The search is closed on the device: one Gram matrix and one statistics pass
    over the benign rows, no pass per probe, no host round trip.  Returns (lambda,
    a float64 device scalar — NaN: a benign row held a NaN and the rows were left
    as they were —, info int32 [2]: status 0 found, 1 threshold reached without
    success (usual with f = 1), 2 no direction (mu == g: the rows become g), 3 not
    finite; and t, the halvings)."""
    M = X if isinstance(X, torch.Tensor) else X.X
    threshold = fang_krum_config(M.shape[0], int(f), threshold)
    return ops.fang_krum_rows(M, int(f), global_flat, threshold)


def fang_trim_config(K: int, f: int, b=2.0) -> float:
    """fang_trim_'s b checked on the host with the shape: finite and > 1 in
    float32, 1 <= f < K."""
    if not 1 <= f < K:
        raise ValueError(f"the trimmed-mean attack needs 1 <= f < K (got f = {f}, K = {K})")
    return ops._fang_trim_b(b)


def fang_trim_(X, f: int, global_flat: torch.Tensor, b: float = 2.0, seed: int = 0, stream: int = 0,
               col0: int = 0) -> None:
    """Fang et al.'s trimmed-mean / median attack, in place on a float32 device
    matrix or a ClientMatrix: per coordinate, rows 0..f-1 <- points just beyond
    the benign rows' (f..K-1) extreme on the side opposite s = sign(mu - g), each
    attacker at a draw of its own between the extreme and the extreme scaled by b
    (the paper's b = 2) away from the benign values; a coordinate with mu == g
    gets mu.  The draws are keyed by (seed, the coordinate's index col0 + k in
    the order the matrix is held in, the attacker, stream): a column range called
    with its own col0 gives the whole call's bits, stream is the round index, and
    a matrix held in another coordinate order draws other values for the same
    parameter."""
    M = X if isinstance(X, torch.Tensor) else X.X
    b = fang_trim_config(M.shape[0], int(f), b)
    ops.fang_trim_rows(M, int(f), global_flat, b, seed, stream, col0)


class Backdoor:
    def __init__(self, trigger_size: int = 3, target_class: int = 0, poison_ratio: float = 0.1,
                 trigger_value: float = 1.0, seed: int = 42, image_size: Tuple[int, int] = (32, 32)):
        self.trigger_size = trigger_size
        self.target_class = target_class
        self.poison_ratio = poison_ratio
        self.trigger_value = trigger_value
        self.seed = seed
        h, w = image_size
        self.position = (h - trigger_size - 1, w - trigger_size - 1)  # 'bottom_right'
        self.num_poisoned = 0
        self.poisoned_indices: List[int] = []

    def choose(self, num_samples: int) -> List[int]:
        np.random.seed(self.seed)
        idx = np.random.choice(list(range(num_samples)), size=int(num_samples * self.poison_ratio),
                               replace=False).tolist()
        self.num_poisoned = len(idx)
        self.poisoned_indices = idx
        return idx

    def apply_trigger_(self, images: torch.Tensor) -> torch.Tensor:
        """images [..., C, H, W] in place."""
        r, c = self.position
        s = self.trigger_size
        images[..., r:r + s, c:c + s] = self.trigger_value
        return images

    def poison_client_(self, images: torch.Tensor, labels: torch.Tensor) -> List[int]:
        """One client's samples flattened in dataset order: images [N, C, H, W],
        labels [N]; poisons them in place and returns the indices."""
        idx = self.choose(images.shape[0])
        if idx:
            sel = torch.tensor(idx, device=images.device)
            sub = images[sel]
            self.apply_trigger_(sub)
            images[sel] = sub
            labels[sel] = self.target_class
        return idx


def poison_batches_(batches, client_cols: Sequence[int], attack: Backdoor) -> None:
    """Poison the resident per-step batches [(images [K,B,...], tokens, labels [K,B])]
    of the client columns `client_cols`: the client's dataset is its samples
    across steps in order (step-major), as a DataLoader over them would see."""
    steps = len(batches)
    for j in client_cols:
        imgs = torch.cat([b[0][j] for b in batches])   # [steps*B, C, H, W]
        labs = torch.cat([b[2][j] for b in batches])
        attack.poison_client_(imgs, labs)
        B = batches[0][0].shape[1]
        for s in range(steps):
            batches[s][0][j].copy_(imgs[s * B:(s + 1) * B])
            batches[s][2][j].copy_(labs[s * B:(s + 1) * B])
