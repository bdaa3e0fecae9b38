"""GPU: the fused strided data gradient (fdgrad_kernel: one launch walks the four
stride-parity classes, sums their split-K ranges in registers and folds the
block's 1x1 shortcut in) against the per-class launches (FLR_DGRAD_FUSED=0) —
bit for bit — and against fp64; dx and the workspace between NaN-pattern margins,
the workspace itself untouched by the fused form.  Both grids of the fused form
(FLR_DGRAD_FUSED_ROWS) run every bit-equality case."""
import functools

import pytest
import torch

from flr import _capi
from flr.nn import _stream

pytestmark = pytest.mark.gpu

K = 3
PAT = 0x7FC0BEEF   # margins, unwritten outputs and the workspace: a quiet NaN no kernel produces
MARGIN = 1024      # int32 words on either side of a buffer
CHANS = [(64, 128), (128, 256), (256, 512)]
SIZES = [2, 4, 8]
BATCHES = [2, 5, 32]
KERNELS = [(3, 1), (1, 0)]   # (KS, pad) at stride 2


def _geom(B, H, Cin, Cout, KS, stride, pad, k=K):
    return (k, B, Cin, H, H, Cout, KS, KS, stride, pad)


def _ho(H, KS, stride, pad):
    return (H + 2 * pad - KS) // stride + 1


@functools.lru_cache(maxsize=4)
def _inputs(B, H, Cin, Cout, KS, stride, pad, k=K):
    """CPU tensors of one shape (the same for every form): dy, w, add, and the
    shortcut's dy and w (Cout channels, 1x1, the conv's stride)."""
    Ho = _ho(H, KS, stride, pad)
    Hs = _ho(H, 1, stride, 0)
    g = torch.Generator(device="cpu").manual_seed(1000 * Cin + 100 * H + 10 * B + KS + stride)
    dy = torch.randn(k * Cout, B, Ho, Ho, generator=g)
    wt = torch.randn(k, KS, KS, Cin, Cout, generator=g) * 0.1
    add = torch.randn(k * Cin, B, H, H, generator=g)
    dys = torch.randn(k * Cout, B, Hs, Hs, generator=g)
    ws = torch.randn(k, 1, 1, Cin, Cout, generator=g) * 0.1
    return dy, wt, add, dys, ws


def _pat(n, cuda):
    return torch.full((n + 2 * MARGIN,), PAT, dtype=torch.int32, device=cuda)


def _margins_ok(buf):
    return bool((buf[:MARGIN] == PAT).all()) and bool((buf[-MARGIN:] == PAT).all())


def _bits(t):
    return t.contiguous().view(torch.int32).cpu()


def _ws_bytes(geom, sgeom):
    n = int(_capi.lib().flr_conv2d_t_workspace(*geom))
    return max(n, int(_capi.lib().flr_conv2d_t_workspace(*sgeom))) if sgeom else n


def _run(cuda, knob, geom, dev, fused, shared=False, add_mode="none", sc=False, check=True):
    """One data gradient through flr_conv2d_bwd_data_t_sc; returns (status, dx bits,
    dx values on the CPU, whether the workspace was written)."""
    knob("FLR_DGRAD_FUSED", "1" if fused else "0")
    k, B, Cin, H, _, Cout, KS, _, stride, pad = geom
    dy, wt, add, dys, wsc = dev
    sgeom = _geom(B, H, Cin, Cout, 1, stride, 0, k) if sc else None
    nb = _ws_bytes(geom, sgeom)
    wsbuf = _pat((nb + 3) // 4, cuda)
    wsp = wsbuf[MARGIN:].data_ptr() if nb else None
    n = k * Cin * B * H * H
    dxbuf = _pat(n, cuda)
    dx = dxbuf[MARGIN:MARGIN + n].view(torch.float32).view(k * Cin, B, H, H)
    addp = None
    if add_mode == "add":
        addp = add.data_ptr()
    elif add_mode == "inplace":
        dx.copy_(add)
        addp = dx.data_ptr()
    rc = _capi.lib().flr_conv2d_bwd_data_t_sc(
        dy.data_ptr(), wt.data_ptr(), 0 if shared else KS * KS * Cin * Cout, addp, dx.data_ptr(), *geom,
        dys.data_ptr() if sc else None, wsc.data_ptr() if sc else None, 0 if shared else Cin * Cout, Cout if sc else 0,
        wsp, nb, _stream(dy))
    torch.cuda.synchronize()
    assert _margins_ok(dxbuf) and _margins_ok(wsbuf)
    out = _bits(dx)
    if check and rc == 0:
        assert not bool((out == PAT).any())  # every element of dx written
    return rc, out, dx.cpu(), bool((wsbuf != PAT).any())


def _splits(geom, nbytes):
    return [int(_capi.lib().flr_conv2d_dgrad_class_splits(*geom, c, nbytes)) for c in range(4)]


def _supported(geom):
    return int(_capi.lib().flr_conv2d_dgrad_fused_supported(*geom))


@pytest.mark.parametrize("KS,pad", KERNELS, ids=["3x3s2", "1x1s2"])
@pytest.mark.parametrize("H", SIZES, ids=lambda h: f"{h}x{h}")
@pytest.mark.parametrize("Cin,Cout", CHANS, ids=lambda c: str(c))
def test_fused_bit_identical_to_per_class(cuda, knob, Cin, Cout, H, KS, pad):
    """Every batch, shared and per-client weights, with and without the addend and
    the folded shortcut; the fused form leaves the workspace untouched (no split-K
    partial is written) where the per-class path fills it whenever a class splits."""
    for B in BATCHES:
        geom = _geom(B, H, Cin, Cout, KS, 2, pad)
        assert _supported(geom) == 1
        dev = tuple(t.to(cuda) for t in _inputs(B, H, Cin, Cout, KS, 2, pad))
        for shared in (False, True):
            for add_mode in ("none", "add"):
                for sc in (False, True):
                    what = (B, shared, add_mode, sc)
                    rc0, ref, _, ws0 = _run(cuda, knob, geom, dev, False, shared, add_mode, sc)
                    knob("FLR_DGRAD_FUSED", "1")
                    assert int(_capi.lib().flr_conv2d_dgrad_fused_preferred(*geom, int(sc))) == 1
                    for rows in ("0", "1"):   # a tile's two class rows in one workgroup / in two
                        knob("FLR_DGRAD_FUSED_ROWS", rows)
                        rc1, got, _, ws1 = _run(cuda, knob, geom, dev, True, shared, add_mode, sc)
                        assert rc0 == 0 and rc1 == 0, what
                        assert torch.equal(ref, got), (what, rows, int((ref != got).sum()))
                        assert not ws1, what
                    knob("FLR_DGRAD_FUSED_ROWS", None)
                    nb = _ws_bytes(geom, _geom(B, H, Cin, Cout, 1, 2, 0) if sc else None)
                    if max(_splits(geom, nb)) > 1:
                        assert ws0, what


def test_split_k_classes_are_covered():
    """The shapes above include, for every class of the 3x3 / 2 conv (1, 2, 2 and 4
    taps) and for the one class of the 1x1 / 2 conv, one whose per-class launch takes
    split-K S > 1 (the planner's own count) — and one where it takes S = 1."""
    seen3 = [set() for _ in range(4)]
    seen1 = set()
    for Cin, Cout in CHANS:
        for H in SIZES:
            for B in BATCHES:
                g3, g1 = _geom(B, H, Cin, Cout, 3, 2, 1), _geom(B, H, Cin, Cout, 1, 2, 0)
                for c, s in enumerate(_splits(g3, _ws_bytes(g3, None))):
                    seen3[c].add(s)
                seen1.add(_splits(g1, _ws_bytes(g1, None))[0])
    for c in range(4):
        assert max(seen3[c]) > 1, (c, seen3[c])
    assert 1 in set().union(*seen3) and 1 in seen1 and max(seen1) > 1, (seen3, seen1)
    # the l3a classes at batch 32 (1, 2, 2, 4 taps) and the l4a classes (2x2 maps: the
    # 3x3 has four live taps, one per class)
    assert _splits(_geom(32, 4, 128, 256, 3, 2, 1), 1 << 30) == [1, 2, 2, 4]
    assert _splits(_geom(32, 2, 256, 512, 3, 2, 1), 1 << 30) == [2, 2, 2, 2]


def test_default_preference(knob):
    """Knob unset (queries only, nothing runs): the fused form where it measured
    faster at 128 clients — l2a, l3a, l4a and the 1x1 shortcuts, alone or with the
    shortcut folded in — and no grid under one column tile per CU (few clients per
    GPU)."""
    knob("FLR_DGRAD_FUSED", None)
    pref = _capi.lib().flr_conv2d_dgrad_fused_preferred
    for Cin, H, Cout in ((64, 8, 128), (128, 4, 256), (256, 2, 512)):
        g3, g1 = (128, 32, Cin, H, H, Cout, 3, 3, 2, 1), (128, 32, Cin, H, H, Cout, 1, 1, 2, 0)
        assert int(pref(*g3, 1)) == 1 and int(pref(*g1, 0)) == 1
        assert int(pref(*g3, 0)) == 1
        assert int(pref(16, *g3[1:], 1)) == 0 and int(pref(3, *g3[1:], 0)) == 0
    knob("FLR_DGRAD_FUSED", "0")
    assert int(pref(128, 32, 64, 8, 8, 128, 3, 3, 2, 1, 1)) == 0
    knob("FLR_DGRAD_FUSED", "1")
    assert int(pref(3, 2, 64, 8, 8, 128, 3, 3, 2, 1, 0)) == 1
    assert int(pref(3, 2, 64, 5, 5, 128, 3, 3, 2, 1, 0)) == 0


def test_fused_without_workspace_matches(cuda, knob):
    """No workspace: the per-class launches fall back to split-K 1, and so does the
    fused form (dgrad_class_splits follows the workspace it is given)."""
    geom = _geom(32, 4, 128, 256, 3, 2, 1)
    assert _splits(geom, 0) == [1, 1, 1, 1]
    dy, wt, add, dys, wsc = (t.to(cuda) for t in _inputs(32, 4, 128, 256, 3, 2, 1))
    outs = []
    for on in ("0", "1"):
        knob("FLR_DGRAD_FUSED", on)
        dx = torch.empty_like(add)
        _capi.call("flr_conv2d_bwd_data_t_sc", dy.data_ptr(), wt.data_ptr(), 9 * 128 * 256, add.data_ptr(),
                   dx.data_ptr(), *geom, dys.data_ptr(), wsc.data_ptr(), 128 * 256, 256, None, 0, _stream(dy))
        torch.cuda.synchronize()
        outs.append(_bits(dx))
    assert torch.equal(*outs)


@pytest.mark.parametrize("KS,pad", KERNELS, ids=["3x3s2", "1x1s2"])
def test_in_place_accumulation(cuda, knob, KS, pad):
    """add == dx.  The 3x3 reaches every class and runs fused in place; the 1x1 skips
    its three empty classes, which the fused form does not do: it keeps the per-class
    launches, and those pixels hold what they held."""
    geom = _geom(5, 4, 64, 128, KS, 2, pad)
    cpu = _inputs(5, 4, 64, 128, KS, 2, pad)
    dev = tuple(t.to(cuda) for t in cpu)
    _, ref, _, _ = _run(cuda, knob, geom, dev, False, add_mode="inplace")
    _, got, val, _ = _run(cuda, knob, geom, dev, True, add_mode="inplace")
    assert torch.equal(ref, got)
    if KS == 1:
        keep = torch.ones(4, 4, dtype=torch.bool)
        keep[0::2, 0::2] = False
        assert torch.equal(_bits(val[:, :, keep]), _bits(cpu[2][:, :, keep]))


INELIGIBLE = [  # (B, H, Cin, Cout, KS, stride, pad)
    (2, 3, 64, 128, 3, 2, 1),   # H = 3: classes of unequal size
    (5, 5, 64, 128, 3, 2, 1),   # H = 5
    (2, 5, 64, 128, 1, 2, 0),   # H = 5, the 1x1 shortcut shape
    (2, 8, 64, 128, 3, 1, 1),   # stride 1: one class
    (2, 8, 64, 128, 3, 4, 1),   # stride 4: sixteen classes
    (2, 4, 96, 128, 3, 2, 1),   # Cin = 96: not a tap-major shape at all
]


@pytest.mark.parametrize("shape", INELIGIBLE, ids=["H3", "H5", "H5-1x1", "stride1", "stride4", "cin96"])
def test_ineligible_shapes_take_the_per_class_path(cuda, knob, shape):
    B, H, Cin, Cout, KS, stride, pad = shape
    geom = _geom(B, H, Cin, Cout, KS, stride, pad)
    assert _supported(geom) == 0
    dev = tuple(t.to(cuda) for t in _inputs(B, H, Cin, Cout, KS, stride, pad))
    for add_mode, sc in (("none", False), ("add", False), ("none", True)):
        rc0, ref, _, _ = _run(cuda, knob, geom, dev, False, add_mode=add_mode, sc=sc, check=False)
        knob("FLR_DGRAD_FUSED", "1")
        assert int(_capi.lib().flr_conv2d_dgrad_fused_preferred(*geom, int(sc))) == 0
        rc1, got, _, _ = _run(cuda, knob, geom, dev, True, add_mode=add_mode, sc=sc, check=False)
        assert rc0 == rc1
        assert rc0 == (0 if Cin % 64 == 0 else -3)   # FLR_ERR_UNSUPPORTED: nothing written
        assert torch.equal(ref, got)
        if rc0 != 0:
            assert bool((ref == PAT).all())


def test_odd_dx_alignment_falls_back(cuda, knob):
    """The fused form stores 8 bytes at a time: a dx that is only 4-byte aligned
    takes the per-class launches, the same bits."""
    geom = _geom(2, 4, 64, 128, 3, 2, 1)
    dy, wt, add, _, _ = (t.to(cuda) for t in _inputs(2, 4, 64, 128, 3, 2, 1))
    nb = _ws_bytes(geom, None)
    ws = torch.empty(max(nb, 4), dtype=torch.uint8, device=cuda)
    outs = []
    for on in ("0", "1"):
        knob("FLR_DGRAD_FUSED", on)
        buf = _pat(add.numel() + 1, cuda)
        dx = buf[MARGIN + 1:MARGIN + 1 + add.numel()].view(torch.float32).view(add.shape)
        assert dx.data_ptr() % 8 == 4
        _capi.call("flr_conv2d_bwd_data_t_ex", dy.data_ptr(), wt.data_ptr(), 9 * 64 * 128, None, dx.data_ptr(), *geom,
                   ws.data_ptr(), nb, _stream(dy))
        torch.cuda.synchronize()
        assert bool((buf[:MARGIN + 1] == PAT).all()) and bool((buf[-MARGIN:] == PAT).all())
        outs.append(_bits(dx))
    assert torch.equal(*outs)


FP64 = [  # (B, H, Cin, Cout, KS, pad, shortcut)
    (5, 8, 64, 128, 3, 1, True),
    (5, 4, 128, 256, 3, 1, False),
    (32, 2, 256, 512, 3, 1, True),
    (5, 4, 256, 512, 1, 0, False),
]


@pytest.mark.parametrize("case", FP64, ids=lambda c: "-".join(str(v) for v in c))
def test_fused_vs_fp64(cuda, knob, case):
    """DESIGN.md §4's layer bar: 2e-6 of the reference's max up to 256-term sums,
    times sqrt(n / 256) past that; n = the most taps x channels one pixel sums
    (class (1, 1)'s four taps, or class (0, 0)'s one tap plus the shortcut), + 1
    for the addend."""
    B, H, Cin, Cout, KS, pad, sc = case
    geom = _geom(B, H, Cin, Cout, KS, 2, pad)
    cpu = _inputs(B, H, Cin, Cout, KS, 2, pad)
    dev = tuple(t.to(cuda) for t in cpu)
    rc, _, dx, _ = _run(cuda, knob, geom, dev, True, add_mode="add", sc=sc)
    assert rc == 0
    dy, wt, add, dys, wsc = (t.double() for t in cpu)

    def ref_dgrad(dyv, wv, ks, p):
        w = wv.permute(0, 4, 3, 1, 2).reshape(K * Cout, Cin, ks, ks)   # torch's [Cout][Cin][kh][kw]
        return torch.nn.grad.conv2d_input((B, K * Cin, H, H), w, dyv.transpose(0, 1), stride=2, padding=p, groups=K)

    ref = ref_dgrad(dy, wt, KS, pad) + add.transpose(0, 1)
    if sc:
        ref = ref + ref_dgrad(dys, wsc, 1, 0)
    taps = 4 if KS == 3 else 1
    n = max(taps * Cout, (Cout if KS == 3 else taps * Cout) + (Cout if sc else 0)) + 1
    tol = 2e-6 * max(1.0, (n / 256) ** 0.5)
    err = (dx.double().transpose(0, 1) - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"fp64: case {case} err {err:.3e} bound {tol * scale:.3e}")
    assert err <= tol * scale, (err, tol * scale)


def test_engine_rows_equal_with_and_without_fused(cuda, knob):
    """flr_train_clients_ex on the full ResNet-18 + GRU model (K = 3, B = 8, two
    steps, dropout masks, one negated row): l2a, l3a and l4a with their shortcuts
    take the fused launch under FLR_DGRAD_FUSED=1; rows, losses and clip norms are
    the per-class launches' bits."""
    from flr import native_trainer as nt
    from flr.models.multimodal import ModelSpec
    from flr.round import initial_global
    from flr.train import TrainConfig, make_dropout_masks, synthetic_batches
    spec, Kc, B, steps = ModelSpec(), 3, 8, 2
    cfg = TrainConfig(local_steps=steps)
    glob = initial_global(spec, 42, cuda)
    batches = synthetic_batches(spec, steps, range(Kc), B, cuda)
    masks = make_dropout_masks(spec, steps, Kc, B, cuda, seed=11)
    rows = []
    for on in ("0", "1"):
        knob("FLR_DGRAD_FUSED", on)
        assert int(_capi.lib().flr_conv2d_dgrad_fused_preferred(Kc, B, 64, 8, 8, 128, 3, 3, 2, 1, 1)) == int(on)
        X, loss, norms = nt.train_clients(spec, glob, batches, cfg, masks, negate_rows=1)
        torch.cuda.synchronize()
        rows.append((X.clone(), loss.clone(), norms.clone()))
    assert torch.isfinite(rows[0][0]).all()
    for a, b in zip(*rows):
        assert torch.equal(a, b)
