"""The robust learning rate's three contracts (include/flr.h: flr_sign_vote,
flr_rlr_apply, flr_rlr_fedavg) restated on the CPU: a row loop in client order
and torch.float32 tensor ops, each its own rounded operation, so no FMA can
arise.  Nothing here has a free summation order: the device results are compared
bit for bit."""
import math

import torch


def fedavg(X, num_examples):
    """flr_fedavg's accumulator: weights (float)n_i, fl(n_i * x) added in client
    order from +0, one division by (float)sum n_i."""
    X = X.float()
    acc = torch.zeros(X.shape[1], dtype=torch.float32)
    for i, n in enumerate(num_examples):
        acc = acc + torch.tensor(float(n), dtype=torch.float32) * X[i]
    return acc / torch.tensor(float(sum(int(n) for n in num_examples)), dtype=torch.float32)


def sign_vote(X, g):
    """int32 [P]: #{k : X[k][p] > g[p]} - #{k : X[k][p] < g[p]}, comparisons only
    (a NaN and -0 against +0 compare false both ways)."""
    votes = torch.zeros(X.shape[1], dtype=torch.int32)
    for k in range(X.shape[0]):
        votes = votes + (X[k] > g).to(torch.int32) - (X[k] < g).to(torch.int32)
    return votes


def rlr_apply(agg, g, votes, theta, eta=1.0):
    """(out, flipped): d = agg - g; out = agg where |votes| >= theta and eta == 1,
    g + eta * d where |votes| >= theta, g - eta * d elsewhere; flipped counts the
    coordinates under the threshold."""
    eta32 = torch.tensor(float(eta), dtype=torch.float32)
    ed = eta32 * (agg - g)
    keep = votes.abs() >= int(theta)
    passed = agg if float(eta32) == 1.0 else g + ed
    return torch.where(keep, passed, g - ed), int((~keep).sum())


def rlr_fedavg(X, num_examples, g, theta, eta=1.0):
    """(out, votes, flipped) of the fused call: the composition, by contract."""
    votes = sign_vote(X, g)
    out, flipped = rlr_apply(fedavg(X, num_examples), g, votes, theta, eta)
    return out, votes, flipped


def resolve_threshold(threshold, K):
    """RobustLRDefense's rule: an int as it is, a float in (0, 1) as
    ceil(threshold * K)."""
    if isinstance(threshold, int):
        return threshold
    return min(K, math.ceil(threshold * K))


def same_bits(a, b):
    """Bit equality of two float32 tensors, any NaN equal to any NaN (their
    payloads are not part of the contract)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = a.isnan(), b.isnan()
    return torch.equal(na, nb) and torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32))
