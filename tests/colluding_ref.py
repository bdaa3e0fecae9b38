"""Reference of the colluding attacks (flr_collude_rows, include/flr.h a16):
torch on the CPU, fp32, the header's arithmetic restated op for op — sequential
row loops over [P] vectors, each torch op one IEEE-rounded fp32 operation (the
square root through float64, see sqrt_rn), so the kernel has to match it bit
for bit."""
import torch

ALIE, IPM = 0, 1


def sqrt_rn(v: torch.Tensor) -> torch.Tensor:
    """The correctly rounded fp32 square root (IEEE 754, the kernel's sqrt_rn).
    torch.sqrt on a float32 CPU tensor is not it: on an MKL build it is the
    vector library's square root, up to 1 ulp off on some 0.7 % of the values of
    a long vector and different from one CPU to the next.  torch.sqrt in
    float64 rounded to float32 is: rounding a square root twice is harmless
    when the wide format has at least 2 * 24 + 2 = 50 significant bits (the
    root of a 24-bit number is never that close to a float32 rounding
    boundary), and float64 has 53 (tests/test_colluding_host.py checks it
    against numpy's sqrt, the hardware instruction)."""
    return torch.sqrt(v.double()).float()


def collude(X: torch.Tensor, nmal: int, mode: int, param: float):
    """X: CPU float32 [K, P].  Returns (matrix, mu, sigma): a copy of X whose
    rows [0, nmal) hold the attack vector, and the benign rows' [nmal, K) mean
    and population standard deviation."""
    assert X.dtype == torch.float32 and X.device.type == "cpu" and X.dim() == 2
    K, P = X.shape
    assert 1 <= nmal < K and mode in (ALIE, IPM)
    nb = torch.tensor(float(K - nmal), dtype=torch.float32)
    par = torch.tensor(param, dtype=torch.float32)
    s = torch.zeros(P, dtype=torch.float32)
    for k in range(nmal, K):
        s = s + X[k]
    mu = s / nb
    q = torch.zeros(P, dtype=torch.float32)
    for k in range(nmal, K):
        d = X[k] - mu
        q = q + d * d
    sigma = sqrt_rn(q / nb)
    vec = mu - par * sigma if mode == ALIE else -(par * mu)
    out = X.clone()
    out[:nmal] = vec
    return out, mu, sigma
