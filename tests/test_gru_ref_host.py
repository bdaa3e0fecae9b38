"""tests/gru_ref.py (the fp64 restatement test_gpu_gru_steps.py holds the GRU
step kernels to) is itself right: its forward step composed over T steps is
torch.nn.GRU, its backward sweep is autograd's gradient of that module, and
its packed layout is a bijection onto the unpadded positions with +0.0
everywhere else and the length flr.nn uses."""
import pytest
import torch

import gru_ref
from flr.nn import _gru_packed

SHAPES = [(3, 4, 5), (2, 1, 1)]  # (B, T, H)
K = 2  # two modules with their own weights: the reference's client axis


def _modules(B, T, H):
    """K torch GRUs whose input projection is the identity (W_ih = I, b_ih = 0),
    so the module's input IS gi and its input gradient is d gi."""
    g = torch.Generator().manual_seed(100 * B + 10 * T + H)
    mods, gis = [], []
    for _ in range(K):
        m = torch.nn.GRU(3 * H, H, num_layers=1, batch_first=True).double()
        with torch.no_grad():
            m.weight_ih_l0.copy_(torch.eye(3 * H, dtype=torch.float64))
            m.bias_ih_l0.zero_()
            m.weight_hh_l0.copy_(torch.randn(3 * H, H, generator=g, dtype=torch.float64))
            m.bias_hh_l0.copy_(torch.randn(3 * H, generator=g, dtype=torch.float64))
        mods.append(m)
        gis.append(torch.randn(B, T, 3 * H, generator=g, dtype=torch.float64).requires_grad_(True))
    dy = torch.randn(K, B, H, generator=g, dtype=torch.float64)
    return mods, gis, dy


def _sweep(gi, whh, bhh, T):
    hs, gates = [torch.zeros(K, gi.shape[1], whh.shape[2], dtype=torch.float64)], []
    for t in range(T):
        r, z, n, hn, h1 = gru_ref.fwd_step(gi[:, :, t], hs[t], whh, bhh)
        gates.append((r, z, n, hn))
        hs.append(h1)
    return hs, gates


@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_fwd_step_composed_is_torch_gru(shape):
    B, T, H = shape
    mods, gis, _ = _modules(B, T, H)
    gi = torch.stack([x.detach() for x in gis])
    whh = torch.stack([m.weight_hh_l0.detach() for m in mods])
    bhh = torch.stack([m.bias_hh_l0.detach() for m in mods])
    hs, _ = _sweep(gi, whh, bhh, T)
    for k, m in enumerate(mods):
        out, hT = m(gis[k])
        assert (hs[T][k] - hT[0]).abs().max().item() <= 1e-12
        for t in range(T):  # every intermediate state, not only the last
            assert (hs[t + 1][k] - out[:, t]).abs().max().item() <= 1e-12


@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_bwd_sweep_is_autograd(shape):
    B, T, H = shape
    mods, gis, dy = _modules(B, T, H)
    gi = torch.stack([x.detach() for x in gis])
    whh = torch.stack([m.weight_hh_l0.detach() for m in mods])
    bhh = torch.stack([m.bias_hh_l0.detach() for m in mods])
    hs, gates = _sweep(gi, whh, bhh, T)
    dgi = torch.zeros_like(gi)
    dwhh, dbhh = torch.zeros_like(whh), torch.zeros_like(bhh)
    dh = dy
    for t in range(T - 1, -1, -1):
        dgh_t, dgi_t, dh_direct = gru_ref.bwd_step(dh, *gates[t], hs[t])
        dgi[:, :, t] = dgi_t
        dwhh += torch.matmul(dgh_t.transpose(1, 2), hs[t])
        dbhh += dgh_t.sum(1)
        dh = gru_ref.bwd_gemm(dh_direct, dgh_t, whh)
    for k, m in enumerate(mods):
        _, hT = m(gis[k])
        (hT[0] * dy[k]).sum().backward()
        for got, want in ((dgi[k], gis[k].grad), (dwhh[k], m.weight_hh_l0.grad), (dbhh[k], m.bias_hh_l0.grad)):
            assert (got - want).abs().max().item() <= 1e-12


PACKS = [(3, 1, 1), (3, 24, 24), (3, 37, 37), (3, 40, 40), (3, 300, 300), (1, 24, 72), (1, 37, 111), (1, 33, 130),
         (1, 1, 3), (1, 300, 900)]  # (NG, H, C)


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("dims", PACKS, ids=[str(d) for d in PACKS])
def test_pack_roundtrip_padding_and_length(dims, trans):
    NG, H, C = dims
    if trans and NG != 1:
        with pytest.raises(ValueError):
            gru_ref.pack(torch.zeros(NG * H * C), NG, H, C, trans)
        return
    g = torch.Generator().manual_seed(NG + 3 * H + 7 * C + trans)
    w = torch.randn(2, NG * H * C, generator=g)
    w[w == 0] = 1.0  # so that a zero in wp is padding
    wp = gru_ref.pack(w, NG, H, C, trans)
    assert wp.shape == (2, _gru_packed(NG, H, C)) and wp.dtype == w.dtype
    assert gru_ref.packed_len(NG, H, C) == _gru_packed(NG, H, C)
    assert torch.equal(gru_ref.unpack(wp, NG, H, C, trans), w)
    bits = wp.view(torch.int32)
    assert int((bits != 0).sum()) == w.numel()          # every element once ...
    assert int((bits == 0).sum()) == wp.numel() - w.numel()  # ... and +0.0 (all bits clear) elsewhere
    assert torch.equal(gru_ref.pack(w[1], NG, H, C, trans), wp[1])  # the one-client form


def test_pack_is_the_documented_fragment_order():
    """The index arithmetic against the formula spelled out as loops."""
    for NG, H, C, trans in ((3, 5, 5, 0), (1, 5, 15, 1), (1, 33, 18, 0), (1, 33, 18, 1)):
        w = torch.arange(1, NG * H * C + 1, dtype=torch.float32)
        nub, S = (H + 31) // 32, (C + 15) // 16
        want = torch.zeros(NG * nub * S * 512)
        for blk in range(NG * nub):
            g, r0 = blk // nub, (blk % nub) * 32
            for s in range(S):
                for q in range(2):
                    for lane in range(64):
                        for e in range(4):
                            row, col = r0 + (lane & 31), 16 * s + 8 * (lane >> 5) + 4 * q + e
                            if row < H and col < C:
                                v = w[col * H + row] if trans else w[(g * H + row) * C + col]
                                want[((blk * S + s) * 2 + q) * 256 + lane * 4 + e] = v
        assert torch.equal(gru_ref.pack(w, NG, H, C, trans), want)
