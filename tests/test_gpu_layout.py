"""a1 / a8 / a15: the negating forms of the round-boundary exports
(flr_broadcast_rows_neg, flr_copy_rows_neg, flr_tap_major_to_torch_neg,
include/flr.h) on the odd sizes, unaligned bases and channel shapes of
test_layout_kernels (tests/test_gpu_train.py), plus aligned ones for the 16-B
paths.  Everything is compared as bit patterns: rows k < nneg are the source
with the sign bit flipped (zeros included), every other row the source, and
the sentinel-filled padding is untouched."""
import numpy as np
import pytest
import torch

from flr import _capi

pytestmark = pytest.mark.gpu

SENT = np.int32(0x7FC12345)
SIGN = np.int32(-2 ** 31)
K = 5
NNEG = [0, 1, K - 1, K, K + 3]
# (n, base offset in floats, row padding): test_layout_kernels' four, then 16-B aligned rows with a tail
# (n % 4 = 3) over more than one workgroup
ROWS = [(7, 0, 9), (1000, 0, 9), (1001, 1, 9), (64, 3, 9), (1000, 0, 12), (4099, 0, 13), (4099, 4, 13)]


def _source(rng, shape):
    s = rng.standard_normal(shape).astype(np.float32)
    flat = s.reshape(-1)
    flat[0] = 0.0
    flat[-1] = -0.0
    return s


def _signed(rows, nneg):
    """rows [K', n] int32 bit patterns, the first nneg with the sign bit flipped."""
    out = rows.copy()
    out[:nneg] ^= SIGN
    return out


def _stream(cuda):
    return torch.cuda.current_stream(cuda).cuda_stream


@pytest.mark.parametrize("n,off,pad", ROWS)
def test_broadcast_rows_neg(cuda, n, off, pad):
    rng = np.random.default_rng(n + off)
    ld = n + pad
    src = np.full(n + off + 2, SENT, np.int32)
    src[off:off + n] = _source(rng, n).view(np.int32)
    d_src = torch.from_numpy(src).to(cuda)
    for nneg in NNEG:
        dst = np.full((K + 1) * ld + off, SENT, np.int32)
        d_dst = torch.from_numpy(dst).to(cuda)
        _capi.call("flr_broadcast_rows_neg", d_src.data_ptr() + 4 * off, n, d_dst.data_ptr() + 4 * off, K, ld, nneg,
                   _stream(cuda))
        torch.cuda.synchronize(cuda)
        want = dst.copy()
        rows = want[off:off + K * ld].reshape(K, ld)
        rows[:, :n] = _signed(np.tile(src[off:off + n], (K, 1)), nneg)
        assert np.array_equal(d_dst.cpu().numpy(), want), nneg
    assert np.array_equal(d_src.cpu().numpy(), src)


@pytest.mark.parametrize("n,off,pad", ROWS)
def test_copy_rows_neg(cuda, n, off, pad):
    rng = np.random.default_rng(n + off + 1)
    sld, dld = n + pad, n + pad + 4 * (off % 2) + off  # the destination's stride differs when the base is offset
    src = np.full(K * sld + off + 2, SENT, np.int32)
    live = _source(rng, (K, n)).view(np.int32)
    src[off:off + K * sld].reshape(K, sld)[:, :n] = live
    d_src = torch.from_numpy(src).to(cuda)
    for nneg in NNEG:
        dst = np.full((K + 1) * dld + off, SENT, np.int32)
        d_dst = torch.from_numpy(dst).to(cuda)
        _capi.call("flr_copy_rows_neg", d_src.data_ptr() + 4 * off, sld, n, d_dst.data_ptr() + 4 * off, dld, K, nneg,
                   _stream(cuda))
        torch.cuda.synchronize(cuda)
        want = dst.copy()
        want[off:off + K * dld].reshape(K, dld)[:, :n] = _signed(live, nneg)
        assert np.array_equal(d_dst.cpu().numpy(), want), nneg
    assert np.array_equal(d_src.cpu().numpy(), src)


# (K, Cout, Cin, k) of test_layout_kernels; (dst offset, row slack): the unaligned 5 / 13 it uses, and a
# 16-B aligned row for the float4 path of the full-tile shapes
@pytest.mark.parametrize("off,pad", [(5, 13), (4, 12)], ids=["unaligned", "aligned"])
@pytest.mark.parametrize("Kc,cout,cin,k", [(3, 64, 64, 3), (2, 70, 20, 3), (2, 128, 64, 1), (1, 5, 3, 2)])
def test_tap_major_to_torch_neg(cuda, Kc, cout, cin, k, off, pad):
    rng = np.random.default_rng(cout * cin + k)
    w = _source(rng, (Kc, cout, cin, k * k))                      # torch order [Cout][Cin][KH*KW] per client
    wt = np.ascontiguousarray(w.transpose(0, 3, 2, 1))             # tap-major [KK][Cin][Cout]
    n = cout * cin * k * k
    ld = n + pad
    d_wt = torch.from_numpy(wt).to(cuda)
    for nneg in sorted({0, 1, Kc - 1, Kc, Kc + 3}):
        dst = np.full((Kc + 1) * ld + off, SENT, np.int32)
        d_dst = torch.from_numpy(dst).to(cuda)
        _capi.call("flr_tap_major_to_torch_neg", d_wt.data_ptr(), Kc, k * k, cin, cout, d_dst.data_ptr() + 4 * off,
                   ld, nneg, _stream(cuda))
        torch.cuda.synchronize(cuda)
        want = dst.copy()
        want[off:off + Kc * ld].reshape(Kc, ld)[:, :n] = _signed(w.reshape(Kc, n).view(np.int32), nneg)
        assert np.array_equal(d_dst.cpu().numpy(), want), nneg
    assert np.array_equal(d_wt.cpu().numpy().view(np.int32), wt.view(np.int32))


def test_nothing_to_copy(cuda):
    """n = 0: FLR_OK, nothing written."""
    buf = np.full(64, SENT, np.int32)
    d_a, d_b = torch.from_numpy(buf).to(cuda), torch.from_numpy(buf).to(cuda)
    _capi.call("flr_broadcast_rows_neg", d_a.data_ptr(), 0, d_b.data_ptr(), K, 8, 2, _stream(cuda))
    _capi.call("flr_copy_rows_neg", d_a.data_ptr(), 8, 0, d_b.data_ptr(), 8, K, 2, _stream(cuda))
    torch.cuda.synchronize(cuda)
    assert np.array_equal(d_b.cpu().numpy(), buf) and np.array_equal(d_a.cpu().numpy(), buf)
