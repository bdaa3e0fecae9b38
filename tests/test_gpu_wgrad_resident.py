"""GPU: the resident form of the tap-major weight gradient (rwgemm_kernel: a
workgroup owns three taps of one split-K part; x and dy are split once per
64-pixel chunk into transposed LDS images and a tap's x fragment is read at the
shifted pixel row) against flr_conv2d_bwd_weight_t_sq with FLR_WGRAD_RESIDENT=0
— dw and the clip-norm slots bit for bit — and against fp64; every buffer
between NaN-pattern margins."""
import pytest
import torch
import torch.nn.functional as F

from flr import _capi
from flr.nn import _stream, _workspace_t

pytestmark = pytest.mark.gpu

K, C = 3, 64
PAT = 0x7FC0BEEF            # margins and unwritten outputs: a quiet NaN no kernel produces
PAT64 = 0x7FF8BEEF7FC0BEEF  # the same for the fp64 clip-norm slots
MARGIN = 1024               # words on either side of a buffer
# (H = W, B).  8x8: B = 2, 3, 5 run split-K 1 with odd image counts; B = 32 is the
# layer1 shape (split-K 2); at B = 33 the two parts are 33 K-tiles each, so the
# boundary cuts image 16 in half — the form handles it (the chunk's images are
# staged whole, only the part's K-tiles are multiplied) and the probe reads 1.
# 4x4 and 2x2: several images per K-tile, B = 9 / 33 leave a short last chunk.
MAPS = [(8, 2), (8, 3), (8, 5), (8, 32), (8, 33), (4, 8), (4, 9), (2, 32), (2, 33)]


def _geom(B, H, Cin=C, Cout=C, KS=3, stride=1, pad=1, k=K):
    return (k, B, Cin, H, H, Cout, KS, KS, stride, pad)


def _guard(t, cuda):
    n = t.numel()
    buf = torch.full((n + 2 * MARGIN,), PAT, dtype=torch.int32, device=cuda)
    view = buf[MARGIN:MARGIN + n].view(torch.float32).view(t.shape)
    view.copy_(t)
    return buf, view


def _out(shape, cuda, dtype=torch.int32):
    n = 1
    for s in shape:
        n *= s
    pat = PAT if dtype == torch.int32 else PAT64
    buf = torch.full((n + 2 * MARGIN,), pat, dtype=dtype, device=cuda)
    ft = torch.float32 if dtype == torch.int32 else torch.float64
    return buf, buf[MARGIN:MARGIN + n].view(ft).view(shape)


def _margins_ok(buf, pat=PAT):
    return bool((buf[:MARGIN] == pat).all()) and bool((buf[-MARGIN:] == pat).all())


def _inputs(geom, seed):
    k, B, Cin, H, W, Cout, KS, _, stride, pad = geom
    Ho = (H + 2 * pad - KS) // stride + 1
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(k * Cin, B, H, W, generator=g)
    dy = torch.randn(k * Cout, B, Ho, Ho, generator=g)
    return x, dy


def _wres_ok(geom):
    return int(_capi.lib().flr_conv2d_wgrad_resident_ok(*geom))


def _run(cuda, knob, geom, tensors, resident, zero_dead=0):
    """flr_conv2d_bwd_weight_t_sq: (dw bits as int32, slot bits as int64, dw values);
    every margin, every promised slot and every dw element checked."""
    knob("FLR_WGRAD_RESIDENT", "1" if resident else "0")
    k, B, Cin, H, W, Cout, KS, _, stride, pad = geom
    bufs = [_guard(t, cuda) for t in tensors]
    (_, x), (_, dy) = bufs
    ws, nb = _workspace_t(geom, cuda)
    wsp = None if ws is None else ws.data_ptr()
    n = int(_capi.lib().flr_conv2d_bwd_weight_t_sq_slots(*geom))
    assert n > 0
    dwbuf, dw = _out((k, KS, KS, Cin, Cout), cuda)
    sqbuf, sq = _out((k, n), cuda, torch.int64)
    _capi.call("flr_conv2d_bwd_weight_t_sq", x.data_ptr(), dy.data_ptr(), dw.data_ptr(), *geom, zero_dead,
               sq.data_ptr(), n, wsp, nb, _stream(x))
    torch.cuda.synchronize()
    for b, _ in bufs:
        assert _margins_ok(b)
    assert _margins_ok(dwbuf) and _margins_ok(sqbuf, PAT64)
    for t, (_, v) in zip(tensors, bufs):  # the inputs are only read
        assert torch.equal(v.contiguous().view(torch.int32).cpu(), t.contiguous().view(torch.int32))
    dwb = dw.contiguous().view(torch.int32).cpu()
    sqb = sq.contiguous().view(torch.int64).cpu()
    assert not bool((dwb == PAT).any())    # every tap is live at these shapes: every element written
    assert not bool((sqb == PAT64).any())  # every promised slot written
    return dwb, sqb, dw.cpu()


def _same(ref, got):
    assert torch.equal(ref[0], got[0]), ("dw", int((ref[0] != got[0]).sum()))
    assert torch.equal(ref[1], got[1]), ("sq", int((ref[1] != got[1]).sum()))


@pytest.mark.parametrize("H,B", MAPS, ids=[f"{h}x{h}-B{b}" for h, b in MAPS])
def test_wgrad_resident_bit_identical_to_default(cuda, knob, H, B):
    geom = _geom(B, H)
    tensors = _inputs(geom, 100 * H + B)
    ref = _run(cuda, knob, geom, tensors, False)
    assert _wres_ok(geom) == 0
    got = _run(cuda, knob, geom, tensors, True)
    assert _wres_ok(geom) == 1  # B = 33 included: a part beginning inside an image is handled
    _same(ref, got)


@pytest.mark.parametrize("H,B", [(2, 32), (8, 3)], ids=["2x2-B32", "8x8-B3"])
def test_wgrad_resident_with_zero_dead_taps(cuda, knob, H, B):
    """No dead tap at these maps: the zero fill has nothing to do and the call still agrees."""
    geom = _geom(B, H)
    tensors = _inputs(geom, 7 * H + B)
    ref = _run(cuda, knob, geom, tensors, False, zero_dead=1)
    got = _run(cuda, knob, geom, tensors, True, zero_dead=1)
    assert _wres_ok(geom) == 1
    _same(ref, got)


@pytest.mark.parametrize("case", ["x-nan-dy-inf", "dy-nan-at-padding"])
def test_wgrad_resident_non_finite_bits(cuda, knob, case):
    """A padding position contributes the same zero operand in both forms: a NaN of dy
    at a corner pixel, times that zero, is a NaN in the taps that read padding there."""
    geom = _geom(3, 8)
    x, dy = _inputs(geom, 7)
    if case == "x-nan-dy-inf":
        x[70, 2, 0, 7] = float("nan")   # client 1, a corner-adjacent edge pixel
        dy[130, 1, 4, 4] = float("inf")
    else:
        dy[130, 1, 0, 0] = float("nan")  # client 2, co 2: taps with kh = 0 or kw = 0 read padding here
    ref = _run(cuda, knob, geom, (x, dy), False)
    got = _run(cuda, knob, geom, (x, dy), True)
    assert _wres_ok(geom) == 1
    assert bool(torch.isnan(got[2]).any())
    if case == "dy-nan-at-padding":
        assert bool(torch.isnan(got[2][2, 0, 0, :, 2]).all())  # NaN x the zero operand
        assert bool(torch.isnan(ref[2][2, 0, 0, :, 2]).all())
    _same(ref, got)


@pytest.mark.parametrize("H,B", [(8, 5), (4, 9)], ids=["8x8-B5", "4x4-B9"])
def test_wgrad_resident_vs_fp64(cuda, knob, H, B):
    """test_gpu_conv.py's bound: 2e-6 of the output's max up to 256 terms, times
    sqrt(n / 256) past that (n = B H W pixels: 320 and 144 here)."""
    geom = _geom(B, H)
    x, dy = _inputs(geom, 31 * H + B)
    _, _, dw = _run(cuda, knob, geom, (x, dy), True)
    assert _wres_ok(geom) == 1
    xd = x.double().transpose(0, 1).contiguous()                        # [B, K*C, H, W]
    wd = torch.zeros(K * C, C, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(xd, wd, stride=1, padding=1, groups=K).backward(dy.double().transpose(0, 1))
    ref = wd.grad.reshape(K, C, C, 3, 3).permute(0, 3, 4, 2, 1)         # [k][kh][kw][ci][co]
    tol = 2e-6 * max(1.0, (B * H * H / 256) ** 0.5)
    err = (dw.double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert err <= tol * max(scale, 1.0), (err, scale)


INELIGIBLE = [  # (B, H, Cin, Cout, KS, stride, pad)
    (2, 8, 64, 128, 3, 1, 1),   # Cout = 128
    (2, 8, 64, 64, 3, 2, 1),    # stride 2
    (2, 16, 64, 64, 3, 1, 1),   # 16x16 maps: an image is larger than the chunk
    (2, 8, 64, 64, 1, 1, 0),    # 1x1 kernel: one tap, nothing staged twice
    (2, 3, 64, 64, 3, 1, 1),    # 3x3 maps: H W = 9 is not 4-aligned and does not divide the chunk
]


@pytest.mark.parametrize("shape", INELIGIBLE, ids=["cout128", "stride2", "16x16", "1x1", "3x3map"])
def test_ineligible_shapes_take_the_default_path(cuda, knob, shape):
    B, H, Cin, Cout, KS, stride, pad = shape
    geom = _geom(B, H, Cin, Cout, KS, stride, pad, k=2)
    tensors = _inputs(geom, sum(shape))
    ref = _run(cuda, knob, geom, tensors, False)
    got = _run(cuda, knob, geom, tensors, True)
    assert _wres_ok(geom) == 0
    _same(ref, got)


def test_engine_rows_equal_with_and_without_wgrad_resident(cuda, knob):
    """Two local steps of the small ResNet + GRU model (64-wide stages: the 8x8, 4x4 and
    2x2 weight gradients take the resident form) through flr_train_clients_ex; the
    norms go through the clip-norm slots."""
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
    rows = []
    for on in ("0", "1"):
        knob("FLR_WGRAD_RESIDENT", on)
        assert _wres_ok((Kc, B, 64, 8, 8, 64, 3, 3, 1, 1)) == int(on)
        X, loss, norms = nt.train_clients(spec, glob, batches, cfg)
        torch.cuda.synchronize()
        rows.append((X.clone(), loss.clone(), norms.clone()))
    assert torch.isfinite(rows[0][0]).all()
    for a, b in zip(*rows):
        assert torch.equal(a, b)
