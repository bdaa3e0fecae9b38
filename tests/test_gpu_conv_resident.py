"""GPU: the resident-B form of the tap-major forward and stride-1 data gradient
(rgemm_kernel: the tile's activation operand split once and kept in LDS across
the kernel taps) against the same entry points with FLR_CONV_RESIDENT=0 — bit
for bit — and against fp64; every buffer between NaN-pattern margins."""
import pytest
import torch
import torch.nn.functional as F

from flr import _capi
from flr.nn import _stream, _workspace_t

pytestmark = pytest.mark.gpu

K, C = 3, 64
PAT = 0x7FC0BEEF   # margins and unwritten outputs: a quiet NaN no kernel produces
MARGIN = 1024      # int32 words on either side of a buffer
# (H = W, B): 128 / (H W) images per tile; the odd batches leave a last tile with
# fewer images (columns past N: zero rows); 8x8 B = 32 is the layer1 shape
MAPS = [(8, 2), (8, 3), (8, 5), (4, 8), (4, 9), (2, 32), (2, 33), (8, 32)]


def _geom(B, H, Cin=C, Cout=C, KS=3, stride=1, pad=1, k=K):
    return (k, B, Cin, H, H, Cout, KS, KS, stride, pad)


def _guard(t, cuda):
    """t's values on the device between two PAT margins: (whole int32 buffer, float view)."""
    n = t.numel()
    buf = torch.full((n + 2 * MARGIN,), PAT, dtype=torch.int32, device=cuda)
    view = buf[MARGIN:MARGIN + n].view(torch.float32).view(t.shape)
    view.copy_(t)
    return buf, view


def _out(shape, cuda):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * MARGIN,), PAT, dtype=torch.int32, device=cuda)
    return buf, buf[MARGIN:MARGIN + n].view(torch.float32).view(shape)


def _margins_ok(buf):
    return bool((buf[:MARGIN] == PAT).all()) and bool((buf[-MARGIN:] == PAT).all())


def _bits(t):
    return t.contiguous().view(torch.int32).cpu()


def _inputs(geom, seed):
    k, B, Cin, H, W, Cout, KS, _, stride, pad = geom
    Ho = (H + 2 * pad - KS) // stride + 1
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(k * Cin, B, H, W, generator=g)
    dy = torch.randn(k * Cout, B, Ho, Ho, generator=g)
    wt = torch.randn(k, KS, KS, Cin, Cout, generator=g) * 0.1
    add = torch.randn(k * Cin, B, H, W, generator=g)
    return x, dy, wt, add


def _run(cuda, knob, geom, tensors, resident, w_stride=None):
    """fwd, dgrad and dgrad + add through the _ex entries; returns the outputs' bits
    and checks every margin."""
    knob("FLR_CONV_RESIDENT", "1" if resident else "0")
    k, B, Cin, H, W, Cout, KS, _, stride, pad = geom
    Ho = (H + 2 * pad - KS) // stride + 1
    if w_stride is None:
        w_stride = KS * KS * Cin * Cout
    bufs = [_guard(t, cuda) for t in tensors]
    (_, x), (_, dy), (_, wt), (_, add) = bufs
    ws, nb = _workspace_t(geom, cuda)
    wsp = None if ws is None else ws.data_ptr()
    ybuf, y = _out((k * Cout, B, Ho, Ho), cuda)
    dxbuf, dx = _out(tuple(x.shape), cuda)
    dxabuf, dxa = _out(tuple(x.shape), cuda)
    st = _stream(x)
    _capi.call("flr_conv2d_fwd_t_ex", x.data_ptr(), wt.data_ptr(), w_stride, y.data_ptr(), *geom, wsp, nb, st)
    _capi.call("flr_conv2d_bwd_data_t_ex", dy.data_ptr(), wt.data_ptr(), w_stride, None, dx.data_ptr(), *geom, wsp,
               nb, st)
    _capi.call("flr_conv2d_bwd_data_t_ex", dy.data_ptr(), wt.data_ptr(), w_stride, add.data_ptr(), dxa.data_ptr(),
               *geom, wsp, nb, st)
    torch.cuda.synchronize()
    for b, _ in bufs:
        assert _margins_ok(b)
    for b in (ybuf, dxbuf, dxabuf):
        assert _margins_ok(b)
    for t, (_, v) in zip(tensors, bufs):  # the inputs are only read
        assert torch.equal(_bits(v), _bits(t))
    outs = tuple(_bits(t) for t in (y, dx, dxa))
    for o in outs:
        assert not bool((o == PAT).any())  # every output element written
    return outs, (y.cpu(), dx.cpu(), dxa.cpu())


def _resident_ok(geom, dgrad):
    return int(_capi.lib().flr_conv2d_resident_ok(*geom, dgrad))


@pytest.mark.parametrize("shared_w", [False, True], ids=["per-client-w", "w_stride0"])
@pytest.mark.parametrize("H,B", MAPS, ids=[f"{h}x{h}-B{b}" for h, b in MAPS])
def test_resident_bit_identical_to_default(cuda, knob, H, B, shared_w):
    geom = _geom(B, H)
    tensors = _inputs(geom, 100 * H + B)
    w_stride = 0 if shared_w else None
    ref, _ = _run(cuda, knob, geom, tensors, False, w_stride)
    assert _resident_ok(geom, 0) == 0 and _resident_ok(geom, 1) == 0
    got, _ = _run(cuda, knob, geom, tensors, True, w_stride)
    assert _resident_ok(geom, 0) == 1 and _resident_ok(geom, 1) == 1
    for which, a, b in zip(("y", "dx", "dx+add"), ref, got):
        assert torch.equal(a, b), (which, int((a != b).sum()))


@pytest.mark.parametrize("case", ["weight-inf-nan", "pixel-nan"])
def test_resident_non_finite_bits(cuda, knob, case):
    """A padding position contributes the same zero operand in both forms, so an inf or
    NaN weight (times that zero) and a NaN pixel give the same NaN patterns."""
    geom = _geom(3, 8)
    x, dy, wt, add = _inputs(geom, 7)
    if case == "weight-inf-nan":
        wt[1, 0, 2, 5, 9] = float("inf")
        wt[2, 1, 1, 40, 33] = float("nan")
    else:
        x[70, 2, 0, 7] = float("nan")   # client 1, a corner-adjacent edge pixel
        dy[130, 1, 4, 4] = float("nan")
    tensors = (x, dy, wt, add)
    ref, _ = _run(cuda, knob, geom, tensors, False)
    got, vals = _run(cuda, knob, geom, tensors, True)
    assert all(bool(torch.isnan(v).any()) for v in vals)
    for which, a, b in zip(("y", "dx", "dx+add"), ref, got):
        assert torch.equal(a, b), (which, int((a != b).sum()))


@pytest.mark.parametrize("H,B", [(8, 5), (4, 9)], ids=["8x8-B5", "4x4-B9"])
def test_resident_vs_fp64(cuda, knob, H, B):
    """test_gpu_conv.py's bound: 2e-6 of the output's max up to 256 terms, times
    sqrt(n / 256) past that (n = 64 * 9 = 576 here)."""
    geom = _geom(B, H)
    x, dy, wt, add = _inputs(geom, 31 * H + B)
    _, (y, dx, dxa) = _run(cuda, knob, geom, (x, dy, wt, add), True)
    assert _resident_ok(geom, 0) == 1 and _resident_ok(geom, 1) == 1
    xd = x.double().transpose(0, 1).contiguous().requires_grad_(True)       # [B, K*C, H, W]
    wd = wt.double().permute(0, 4, 3, 1, 2).reshape(K * C, C, 3, 3)         # torch's [Cout][Cin][kh][kw]
    yr = F.conv2d(xd, wd, stride=1, padding=1, groups=K)
    yr.backward(dy.double().transpose(0, 1))
    dxr = xd.grad
    tol = 2e-6 * max(1.0, (C * 9 / 256) ** 0.5)
    for which, got, ref in (("y", y, yr.detach()), ("dx", dx, dxr), ("dx+add", dxa, dxr + add.double().transpose(0, 1))):
        err = (got.double().transpose(0, 1) - ref).abs().max().item()
        scale = ref.abs().max().item()
        assert err <= tol * max(scale, 1.0), (which, err, scale)


INELIGIBLE = [  # (B, H, Cin, Cout, KS, stride, pad)
    (2, 8, 64, 128, 3, 1, 1),   # Cout = 128: the forward's M, the data gradient's reduction channels
    (2, 8, 64, 64, 3, 2, 1),    # stride 2
    (2, 16, 64, 64, 3, 1, 1),   # 16x16 maps: an image is wider than the tile
    (2, 8, 64, 64, 1, 1, 0),    # 1x1 kernel: one tap, nothing staged twice
]


@pytest.mark.parametrize("shape", INELIGIBLE, ids=["cout128", "stride2", "16x16", "1x1"])
def test_ineligible_shapes_take_the_default_path(cuda, knob, shape):
    B, H, Cin, Cout, KS, stride, pad = shape
    geom = _geom(B, H, Cin, Cout, KS, stride, pad, k=2)
    tensors = _inputs(geom, sum(shape))
    ref, _ = _run(cuda, knob, geom, tensors, False)
    got, _ = _run(cuda, knob, geom, tensors, True)
    assert _resident_ok(geom, 0) == 0 and _resident_ok(geom, 1) == 0
    for a, b in zip(ref, got):
        assert torch.equal(a, b)


def test_engine_rows_equal_with_and_without_resident(cuda, knob):
    """One local update of the small ResNet + GRU model (64-wide stages: layer1 at
    8x8, then 4x4 and 2x2 maps take the resident form) through flr_train_clients_ex."""
    from flr import native_trainer as nt
    from flr.models.multimodal import ModelSpec
    from flr.round import initial_global
    from flr.train import TrainConfig, synthetic_batches
    spec = ModelSpec(widths=(64, 64, 64, 64), blocks=(1, 1, 1, 1), vocab=50, embed=8, hidden=16, fusion=16,
                     dropout=0.0)
    Kc, B, steps = 2, 32, 2
    cfg = TrainConfig(local_steps=steps)
    glob = initial_global(spec, 42, cuda)
    batches = synthetic_batches(spec, steps, range(Kc), B, cuda)
    assert _resident_ok((Kc, B, 64, 8, 8, 64, 3, 3, 1, 1), 0) == 1
    rows = []
    for on in ("0", "1"):
        knob("FLR_CONV_RESIDENT", on)
        X, loss, norms = nt.train_clients(spec, glob, batches, cfg)
        torch.cuda.synchronize()
        rows.append((X.clone(), loss.clone(), norms.clone()))
    assert torch.isfinite(rows[0][0]).all()
    for a, b in zip(*rows):
        assert torch.equal(a, b)
