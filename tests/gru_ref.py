"""The GRU step kernels' operations restated plainly (csrc/train_gru.hip,
include/flr.h "a3: GRU recurrence"): one time step of torch's GRU cell forward
and backward for K clients at once, the backward's recurrence GEMM, and the
fused kernels' packed weight layout.  Everything runs in the dtype it is given
(the tests pass fp64); test_gru_ref_host.py pins it to torch.nn.GRU and autograd.

Layouts per step (the kernels' layouts with the time axis taken out):
  gi_t, dgi_t, dgh_t [K][B][3H] (gates r, z, n), h, r, z, n, hn, dy [K][B][H],
  whh [K][3H][H], bhh [K][3H]."""
import torch


def fwd_step(gi_t, h, whh, bhh):
    """(r, z, n, hn, h_next) of torch's cell: gh = h W_hh^T + b_hh,
    r = sigmoid(i_r + h_r), z = sigmoid(i_z + h_z), hn = h_n (bias included),
    n = tanh(i_n + r * hn), h' = (h - n) * z + n."""
    H = h.shape[-1]
    gh = torch.matmul(h, whh.transpose(1, 2)) + bhh[:, None, :]
    r = torch.sigmoid(gi_t[..., :H] + gh[..., :H])
    z = torch.sigmoid(gi_t[..., H:2 * H] + gh[..., H:2 * H])
    hn = gh[..., 2 * H:]
    n = torch.tanh(gi_t[..., 2 * H:] + r * hn)
    return r, z, n, hn, (h - n) * z + n


def bwd_step(dy, r, z, n, hn, h_prev):
    """(dgh_t, dgi_t, dh_direct) for dy = dL/dh_{t+1}: the derivative with
    respect to gh = h_t W_hh^T + b_hh, to gi[:, :, t], and the part of dL/dh_t
    that does not pass through W_hh (the z-gate path, dy * z)."""
    dz = dy * (h_prev - n)
    dn = dy * (1.0 - z)
    dnp = dn * (1.0 - n * n)       # through tanh
    drp = dnp * hn * (r * (1.0 - r))  # through r's sigmoid
    dzp = dz * (z * (1.0 - z))
    return torch.cat([drp, dzp, dnp * r], -1), torch.cat([drp, dzp, dnp], -1), dy * z


def bwd_gemm(dh_direct, dgh_t, whh):
    """dL/dh_t = dh_direct + dgh_t W_hh."""
    return dh_direct + torch.matmul(dgh_t, whh)


def abs_products(a, W):
    """sum_r |a[k][i][r]| |W[k][j][r]| for every output element [k][i][j] of
    a W^T: the scale of that sum's rounding error in any summation order."""
    return torch.matmul(a.abs(), W.abs().transpose(1, 2))


def packed_len(NG, H, C):
    return NG * ((H + 31) // 32) * ((C + 15) // 16) * 512


def _pack_index(NG, H, C, trans):
    """For every packed position: the flat source offset in one client's w and
    whether the position holds an element (False: zero padding).
      wp[((blk*S + s)*2 + q)*256 + lane*4 + e] = M[blk row (lane & 31)][16 s + 8 (lane >> 5) + 4 q + e]
    with blk over NG * ceil(H/32) (group g = blk // nub, rows 32 (blk % nub) ..)
    and S = ceil(C/16); M[(g, r)][c] = w[(g H + r) C + c] (trans = 0) or
    w[c H + r] (trans = 1, NG = 1: the transpose of a [C][H] matrix)."""
    if trans and NG != 1:
        raise ValueError("trans = 1 packs one group")
    nub, S = (H + 31) // 32, (C + 15) // 16
    o = torch.arange(NG * nub * S * 512, dtype=torch.int64)
    e, lane, q = o % 4, (o // 4) % 64, (o // 256) % 2
    s, blk = (o // 512) % S, o // (512 * S)
    g, row = blk // nub, (blk % nub) * 32 + (lane & 31)
    col = 16 * s + 8 * (lane >> 5) + 4 * q + e
    ok = (row < H) & (col < C)
    src = col * H + row if trans else (g * H + row) * C + col
    return torch.where(ok, src, torch.zeros_like(src)), ok


def pack(w, NG, H, C, trans):
    """w: [K, NG*H*C] (or any shape with that many elements per leading index;
    1-D for one client) -> [K, packed_len] (1-D for 1-D input), +0.0 in every
    padded position, the elements' bits unchanged."""
    one = w.dim() == 1
    flat = w.reshape(1 if one else w.shape[0], NG * H * C)
    src, ok = _pack_index(NG, H, C, trans)
    wp = torch.where(ok[None, :], flat[:, src], torch.zeros((), dtype=w.dtype))
    return wp[0] if one else wp


def unpack(wp, NG, H, C, trans):
    """The inverse of pack: [K, packed_len] -> [K, NG*H*C] (1-D for 1-D input)."""
    one = wp.dim() == 1
    flat = wp.reshape(1 if one else wp.shape[0], packed_len(NG, H, C))
    src, ok = _pack_index(NG, H, C, trans)
    w = torch.empty(flat.shape[0], NG * H * C, dtype=wp.dtype)
    w[:, src[ok]] = flat[:, ok]
    return w[0] if one else w
