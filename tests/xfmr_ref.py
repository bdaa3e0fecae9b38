"""Reference model of the encoder kernels of csrc/train_xfmr.hip in plain
torch: attention, LayerNorm and the embedding gradient, forwards and
closed-form backwards (no autograd in here).  A helper module, not a test file;
tests/test_xfmr_ref_host.py pins it to torch's own autograd, F.layer_norm and
F.embedding.

Everything computes in ``dtype`` (fp64 by default).  The GPU tests also run the
same formulas in fp32 on the CPU: that evaluation's error against the fp64 one
is the yardstick for the bounds the project's fixed ones do not cover."""
import math

import torch


def _heads(t, H):
    """[..., T, H * dh] -> [..., H, T, dh]"""
    *lead, T, D = t.shape
    return t.reshape(*lead, T, H, D // H).transpose(-3, -2)


def _merge(t):
    """[..., H, T, dh] -> [..., T, H * dh]"""
    *lead, H, T, dh = t.shape
    return t.transpose(-3, -2).reshape(*lead, T, H * dh)


def _qkv(qkv, H, dtype):
    D = qkv.shape[-1] // 3
    x = qkv.to(dtype)
    return tuple(_heads(x[..., i * D:(i + 1) * D], H) for i in range(3))


def _softmax(q, k):
    """P [..., H, T, T] and lse [..., H, T] of S = q k^T / sqrt(dh), the row
    maximum subtracted before the exponential."""
    s = q @ k.transpose(-2, -1) / math.sqrt(q.shape[-1])
    m = s.max(-1, keepdim=True).values
    p = torch.exp(s - m)
    z = p.sum(-1, keepdim=True)
    return p / z, (m + torch.log(z)).squeeze(-1)


def attention_ref(qkv, H, dtype=torch.float64):
    """qkv [..., T, 3D] (q | k | v, each H heads of D / H columns) ->
    ctx [..., T, D] (heads concatenated), lse [..., H, T]."""
    q, k, v = _qkv(qkv, H, dtype)
    p, lse = _softmax(q, k)
    return _merge(p @ v), lse


def attention_bwd_ref(qkv, dctx, H, dtype=torch.float64):
    """-> dq, dk, dv, each [..., T, D]:
    dV = P^T dO; dP = dO V^T; dS = P (dP - rowsum(dO O)) / sqrt(dh);
    dQ = dS K; dK = dS^T Q."""
    q, k, v = _qkv(qkv, H, dtype)
    p, _ = _softmax(q, k)
    do = _heads(dctx.to(dtype), H)
    o = p @ v
    dv = p.transpose(-2, -1) @ do
    dp = do @ v.transpose(-2, -1)
    drow = (do * o).sum(-1, keepdim=True)
    ds = p * (dp - drow) / math.sqrt(q.shape[-1])
    return _merge(ds @ k), _merge(ds.transpose(-2, -1) @ q), _merge(dv)


def layernorm_ref(x, gamma, beta, eps, residual=None, dtype=torch.float64):
    """x / residual [K, R, D], gamma / beta [K, D] -> y, s, mean, rstd with
    s = x [+ residual] rounded in the inputs' own dtype (LayerNorm's input is
    that tensor), the biased variance about the mean (two passes) and
    rstd = 1 / sqrt(var + eps); mean / rstd [K, R]."""
    s = (x if residual is None else x + residual).to(dtype)
    mean = s.mean(-1, keepdim=True)
    d = s - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = d * rstd * gamma.to(dtype).unsqueeze(1) + beta.to(dtype).unsqueeze(1)
    return y, s, mean.squeeze(-1), rstd.squeeze(-1)


def layernorm_bwd_ref(dy, s, gamma, mean, rstd, dskip=None, dtype=torch.float64):
    """-> dx (= ds, the gradient of both x and the residual), dgamma, dbeta:
    xh = (s - mean) rstd; gy = gamma dy;
    dx = rstd (gy - mean(gy) - xh mean(gy xh)) [+ dskip];
    dgamma = sum_rows dy xh; dbeta = sum_rows dy."""
    dy, s = dy.to(dtype), s.to(dtype)
    mean, rstd = mean.to(dtype).unsqueeze(-1), rstd.to(dtype).unsqueeze(-1)
    xh = (s - mean) * rstd
    gy = gamma.to(dtype).unsqueeze(1) * dy
    dx = rstd * (gy - gy.mean(-1, keepdim=True) - xh * (gy * xh).mean(-1, keepdim=True))
    if dskip is not None:
        dx = dx + dskip.to(dtype)
    return dx, (dy * xh).sum(1), dy.sum(1)


def embedding_bwd_ref(ids, dout, V):
    """dtable [V, E] of one client: from 0, dtable[ids[n]] += dout[n] for
    n = 0, 1, ... in position order, every addition rounded in dout's dtype
    (torch's CPU embedding_dense_backward, bit for bit).  ids [N] must lie in
    [0, V): the kernels skip the others, so a caller drops them first."""
    dt = torch.zeros(V, dout.shape[-1], dtype=dout.dtype)
    for n, i in enumerate(ids.tolist()):
        dt[i] += dout[n]
    return dt


def rel_by_slice(a, ref, slices):
    """max over the slices (indices into both tensors) of
    max|a - ref| / max|ref|: a wrong slice of small magnitude does not hide
    behind a large one."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    worst = 0.0
    for sl in slices:
        x, r = a[sl], ref[sl]
        worst = max(worst, ((x - r).abs().max() / r.abs().max().clamp_min(1e-30)).item())
    return worst


WHOLE = [...]  # rel_by_slice's slices for one tensor as a whole


def head_slices(H, dh, parts=1):
    """Column slices of a [..., parts * H * dh] tensor, one per (part, head):
    ctx (parts = 1) or dqkv (parts = 3: dq, dk, dv per head)."""
    return [(..., slice((p * H + h) * dh, (p * H + h + 1) * dh)) for p in range(parts) for h in range(H)]
