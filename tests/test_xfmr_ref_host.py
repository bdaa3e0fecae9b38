"""tests/xfmr_ref.py (the restatement test_gpu_xfmr_edges.py holds the encoder
kernels to) is itself right: its attention and LayerNorm forwards are torch's,
their closed-form backwards are autograd's gradients, its embedding gradient is
F.embedding's bit for bit, and rel_by_slice is the per-slice maximum."""
import math

import pytest
import torch
import torch.nn.functional as F

import xfmr_ref

RTOL = 1e-12


def _close(a, b):
    return (a - b).abs().max().item() <= RTOL * max(b.abs().max().item(), 1.0)


@pytest.mark.parametrize("T,H,dh", [(1, 1, 64), (5, 3, 64), (33, 2, 64), (7, 2, 8)])
def test_attention_is_torch_softmax_attention_and_autograd(T, H, dh):
    K, B, D = 2, 2, H * dh
    g = torch.Generator().manual_seed(T + H)
    qkv = torch.randn(K, B, T, 3 * D, generator=g, dtype=torch.float64).requires_grad_(True)
    dctx = torch.randn(K, B, T, D, generator=g, dtype=torch.float64)
    q, k, v = qkv.view(K, B, T, 3, H, dh).permute(3, 0, 1, 4, 2, 5)
    s = q @ k.transpose(-2, -1) / math.sqrt(dh)
    want = (torch.softmax(s, -1) @ v).transpose(2, 3).reshape(K, B, T, D)
    (dwant,) = torch.autograd.grad(want, qkv, dctx)
    ctx, lse = xfmr_ref.attention_ref(qkv.detach(), H)
    assert ctx.shape == (K, B, T, D) and lse.shape == (K, B, H, T)
    assert _close(ctx, want.detach())
    assert _close(lse, torch.logsumexp(s.detach(), -1))
    dq, dk, dv = xfmr_ref.attention_bwd_ref(qkv.detach(), dctx, H)
    assert _close(torch.cat([dq, dk, dv], -1), dwant)


def test_attention_large_scores_stay_finite():
    """The reference subtracts the row maximum: scores far past exp's range."""
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn(1, 9, 3 * 64, generator=g, dtype=torch.float64) * 40
    ctx, lse = xfmr_ref.attention_ref(qkv, 1)
    q, k, v = qkv[0].split(64, -1)
    s = q @ k.T / 8
    assert s.abs().max() > 1000 and torch.isfinite(ctx).all() and torch.isfinite(lse).all()
    assert _close(ctx[0], torch.softmax(s, -1) @ v) and _close(lse[0, 0], torch.logsumexp(s, -1))


@pytest.mark.parametrize("R,D,res", [(1, 4, False), (5, 12, True), (66, 260, True), (3, 1024, False)])
@pytest.mark.parametrize("eps", [1e-5, 1e-12])
def test_layernorm_is_f_layer_norm_and_autograd(R, D, res, eps):
    K = 2
    g = torch.Generator().manual_seed(R + D)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, r = rnd(K, R, D) * 2 + 0.5, (rnd(K, R, D) if res else None)
    gam, bet, dy, dsk = 1 + 0.1 * rnd(K, D), 0.1 * rnd(K, D), rnd(K, R, D), (rnd(K, R, D) if res else None)
    leaves = [t.clone().requires_grad_(True) for t in (x, r, gam, bet) if t is not None]
    xs = leaves[0] + leaves[1] if res else leaves[0]
    want = torch.stack([F.layer_norm(xs[k], (D,), leaves[-2][k], leaves[-1][k], eps) for k in range(K)])
    outs, gos = ([want, xs], [dy, dsk]) if res else ([want], [dy])
    grads = torch.autograd.grad(outs, leaves, gos)
    y, s, mean, rstd = xfmr_ref.layernorm_ref(x, gam, bet, eps, residual=r)
    assert _close(y, want.detach()) and _close(s, xs.detach())
    assert _close(mean, xs.detach().mean(-1))
    assert _close(rstd, 1 / torch.sqrt(xs.detach().var(-1, unbiased=False) + eps))
    dx, dgam, dbet = xfmr_ref.layernorm_bwd_ref(dy, s, gam, mean, rstd, dskip=dsk)
    assert _close(dx, grads[0])
    if res:
        assert _close(dx, grads[1])  # the residual's gradient is the same tensor
    assert _close(dgam, grads[-2]) and _close(dbet, grads[-1])


@pytest.mark.parametrize("V,E,N", [(11, 4, 1), (7, 12, 5), (50, 8, 300), (3, 260, 64)])
def test_embedding_bwd_is_f_embedding_bitexact(V, E, N):
    g = torch.Generator().manual_seed(V + N)
    ids = torch.randint(0, V, (N,), generator=g)
    ids[: N // 4] = ids[0]  # a long run: the order of the additions shows
    dout = torch.randn(N, E, generator=g)
    table = torch.randn(V, E, generator=g).requires_grad_(True)
    (want,) = torch.autograd.grad(F.embedding(ids, table), table, dout)
    got = xfmr_ref.embedding_bwd_ref(ids, dout, V)
    assert got.dtype == torch.float32 and torch.equal(got, want)


def test_rel_by_slice_takes_the_worst_slice():
    ref = torch.zeros(2, 8)
    ref[:, :4], ref[:, 4:] = 100.0, 0.01
    a = ref.clone()
    a[1, 5] += 0.001  # 10 % of its slice, 1e-5 of the global maximum
    slices = xfmr_ref.head_slices(2, 4)
    assert slices == [(..., slice(0, 4)), (..., slice(4, 8))]
    assert abs(xfmr_ref.rel_by_slice(a, ref, slices) - 0.1) < 1e-6
    assert abs(xfmr_ref.rel_by_slice(a, ref, xfmr_ref.WHOLE) - 1e-5) < 1e-10
    assert xfmr_ref.rel_by_slice(ref, ref, slices) == 0.0
    assert [s[1] for s in xfmr_ref.head_slices(2, 4, parts=3)] == [slice(4 * i, 4 * i + 4) for i in range(6)]
