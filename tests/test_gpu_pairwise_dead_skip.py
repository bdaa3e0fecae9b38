"""GPU: the dead regions of the reference-exact Krum distances
(flr_pairwise_l2_reference_tap_dead, FLR_REF_DEAD_SKIP): a 3 x 3 block whose
dead taps every row shares runs as a live stream plus one shared dead stream,
and the same-kind pairs skip their dead steps.

Every case follows test_reference_mode_deferred_dead_taps: the rows have NaN
holes where the dead slabs are, and D must equal, bit for bit, the C oracle's D
(oracle.normref, the reference's torch.norm restated) of the matrix with the
slabs filled in, in the reference's coordinate order — with the dead regions
(default) and without them (FLR_REF_DEAD_SKIP=0)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import normref
from flr import ops
from flr.matrix import padded_ld

pytestmark = pytest.mark.gpu

ONE = 0x1EF   # one live tap: the centre
FOUR = 0x04F  # four live taps: 4, 5, 7, 8


def _case(K, blocks, masks, nneg, tail, seed, g_edit=None, x_edit=None):
    """(holes on the device [K, ld], g on the device, P, the oracle's D).
    g_edit(g, dead_index): edits g (training order) given the indices of its
    dead coordinates; x_edit(X): edits the reference-order rows (live values)."""
    P = max(o + co * ci * kk for o, co, ci, kk in blocks) + tail
    gen = torch.Generator().manual_seed(seed)
    X = torch.randn(K, P, generator=gen) * 0.05
    X[: K // 5] = -X[: K // 5]
    X += 1e-3 * torch.randn(K, P, generator=gen) * torch.exp(torch.randn(K, P, generator=gen))
    if x_edit is not None:
        x_edit(X)
    g = torch.randn(P, generator=gen)
    dead_cols = []
    for (o, co, ci, kk), m in zip(blocks, masks):
        for t in range(kk):
            if m >> t & 1:
                dead_cols.append(torch.arange(o + t * ci * co, o + (t + 1) * ci * co))
    dead_cols = torch.cat(dead_cols)
    if g_edit is not None:
        g_edit(g, dead_cols)
    train = X.clone()
    for o, co, ci, kk in blocks:
        w = X[:, o:o + co * ci * kk].reshape(K, co, ci, kk)
        train[:, o:o + co * ci * kk] = w.permute(0, 3, 2, 1).reshape(K, -1)
    filled, holes = train.clone(), train.clone()
    filled[:, dead_cols] = g[dead_cols]
    filled[:nneg, dead_cols] = -g[dead_cols]
    holes[:, dead_cols] = float("nan")
    ref = filled.clone()  # the filled matrix in the reference's order
    for o, co, ci, kk in blocks:
        w = filled[:, o:o + co * ci * kk].reshape(K, kk, ci, co)
        ref[:, o:o + co * ci * kk] = w.permute(0, 3, 2, 1).reshape(K, -1)
    want = normref.distance_matrix(ref.numpy())
    data = torch.zeros((K, padded_ld(P)), dtype=torch.float32)
    data[:, :P] = holes
    return data.cuda(), g.cuda(), P, want


def _both(knob, data, g, P, blocks, masks, nneg, want):
    for skip in ("1", "0"):
        knob("FLR_REF_DEAD_SKIP", skip)
        D = ops.pairwise_l2(data[:, :P], "reference", tap_blocks=blocks, dead=(masks, g, nneg)).cpu().numpy()
        assert np.array_equal(D, want, equal_nan=True), (skip, np.argwhere(~np.isclose(D, want, rtol=0, atol=0,
                                                                                      equal_nan=True))[:8])


@pytest.mark.parametrize("blocks,masks", [
    ([(64, 32, 32, 9)], [ONE]),      # mixed and same-kind lanes in one wave, a tail with no dead tap
    ([(64, 64, 32, 9)], [FOUR]),
], ids=["one_live", "four_live"])
def test_dead_skip_one_block(cuda, knob, blocks, masks):
    K, nneg = 40, 5
    data, g, P, want = _case(K, blocks, masks, nneg, 43, 7)
    assert np.isfinite(want).all()
    _both(knob, data, g, P, blocks, masks, nneg, want)


@pytest.mark.parametrize("blocks", [
    [(64, 36, 33, 9), (64 + 36 * 33 * 9 + 24, 32, 32, 9)],  # the second at off % 8 == 4
    [(64, 32, 32, 9), (64 + 9216 + 24, 32, 32, 9)],         # both at off % 8 == 0: three plain steps between
], ids=["off4", "off0"])
def test_dead_skip_two_blocks_24_apart(cuda, knob, blocks):
    K, nneg = 40, 5
    assert blocks[1][0] - (blocks[0][0] + blocks[0][1] * blocks[0][2] * 9) == 24
    data, g, P, want = _case(K, blocks, [ONE, FOUR], nneg, 43, 8)
    _both(knob, data, g, P, blocks, [ONE, FOUR], nneg, want)


@pytest.mark.parametrize("K", [33, 70])
@pytest.mark.parametrize("which", ["0", "1", "K-1", "K"])
def test_dead_skip_nneg_edges(cuda, knob, K, which):
    """K = 33: a diagonal super-block with its antipodal pairs and a ragged
    second one; K = 70: three super-blocks, mixed off-diagonal tiles."""
    nneg = {"0": 0, "1": 1, "K-1": K - 1, "K": K}[which]
    blocks, masks = [(64, 32, 32, 9)], [ONE]
    data, g, P, want = _case(K, blocks, masks, nneg, 43, 9 + K)
    _both(knob, data, g, P, blocks, masks, nneg, want)


def test_dead_skip_segmented(cuda, knob):
    """A workspace too small for one segment (what FLR_REF_WS_CAP does to
    ops.pairwise_l2; flr.ops reads that variable once, at import, so the capped
    workspace is passed to the library here): room for 1536 chain steps of the
    2325, two segments of 1536; the first dead block, steps 8 .. 1159, lies
    inside the first segment (a dead region), the second, steps 1168 .. 2319,
    crosses the segment end (expanded as before, in both segments)."""
    from flr import _capi
    K, nneg = 16, 3
    blocks, masks = [(64, 32, 32, 9), (64 + 9216 + 64, 32, 32, 9)], [ONE, ONE]
    data, g, P, want = _case(K, blocks, masks, nneg, 43, 11)
    lib = _capi.lib()
    a_bytes = (8 * K * K * 4 + 255) // 256 * 256
    nbytes = a_bytes + K * 32 * 2560 + 4096 + 256
    assert nbytes < int(lib.flr_pairwise_l2_reference_workspace(K, P))
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=cuda)
    wp = (ws.data_ptr() + 255) // 256 * 256
    taps = [v for b in blocks for v in b]
    tarr = (ctypes.c_int64 * len(taps))(*taps)
    marr = (ctypes.c_uint64 * len(masks))(*masks)
    st = torch.cuda.current_stream().cuda_stream
    for skip in ("1", "0"):
        knob("FLR_REF_DEAD_SKIP", skip)
        D = torch.empty((K, K), dtype=torch.float64, device=cuda)
        _capi.call("flr_pairwise_l2_reference_tap_dead", data.data_ptr(), K, P, data.stride(0),
                   ctypes.addressof(tarr), len(blocks), ctypes.addressof(marr), g.data_ptr(), nneg, D.data_ptr(), wp,
                   nbytes, 0, 1, st)
        torch.cuda.synchronize()
        assert np.array_equal(D.cpu().numpy(), want), skip


def _one_inf(g, dead):
    g[dead[1234]] = float("inf")


def _one_nan(g, dead):
    g[dead[4321]] = float("nan")


def _signed_zeros(g, dead):
    g[dead[0::2]] = 0.0
    g[dead[1::2]] = -0.0


def _live_nan(X):
    X[4, 64 + 9 * 500 + 4] = float("nan")  # the live (centre) tap of row 4


def _huge(g, dead):
    g[dead[[5, 777, 4000]]] = torch.tensor([1e19, -1e19, 1e19])


@pytest.mark.parametrize("g_edit,x_edit", [(_one_inf, None), (_one_nan, None), (None, _live_nan),
                                           (_signed_zeros, None), (_huge, None)],
                         ids=["dead_inf", "dead_nan", "live_nan", "signed_zeros", "overflow"])
def test_dead_skip_non_finite(cuda, knob, g_edit, x_edit):
    """A dead value of g that is not finite makes every same-kind pair NaN
    (inf - inf), a NaN one every pair; a live NaN its row's pairs; dead values
    of +-0 and of magnitude 1e19 ((2 g)^2 overflows to inf on the mixed pairs)
    leave the same-kind pairs finite."""
    K, nneg = 9, 3
    blocks, masks = [(64, 32, 32, 9)], [ONE]
    data, g, P, want = _case(K, blocks, masks, nneg, 43, 13, g_edit, x_edit)
    off = ~np.eye(K, dtype=bool)
    same = np.equal.outer(np.arange(K) < nneg, np.arange(K) < nneg) & off
    if g_edit is _one_inf:
        assert np.isnan(want[same]).all() and np.isinf(want[~same & off]).all()
    elif g_edit is _one_nan:
        assert np.isnan(want[off]).all()
    elif x_edit is _live_nan:
        assert np.isnan(want[4, off[4]]).all() and np.isfinite(np.delete(np.delete(want, 4, 0), 4, 1)).all()
    elif g_edit is _huge:
        assert np.isfinite(want[same]).all() and np.isinf(want[~same & off]).all()
    else:
        assert np.isfinite(want).all()
    _both(knob, data, g, P, blocks, masks, nneg, want)


def test_dead_skip_whole_round(cuda, knob):
    """Two sign-flip rounds of the small spec of test_reference_mode_round_engine:
    the global model is the same with the dead regions and without."""
    from flr.models.multimodal import TINY
    from flr.round import RoundConfig, RoundEngine
    from flr.train import TrainConfig
    out = []
    for skip in ("1", "0"):
        knob("FLR_REF_DEAD_SKIP", skip)
        rc = RoundConfig(num_clients=12, batch=4, defense="krum", num_attackers=2, attack="sign_flip",
                         defense_cfg={"pairwise_method": "reference"})
        eng = RoundEngine(TINY, rc, TrainConfig(local_steps=2), cuda)
        eng.run_round()
        eng.run_round()
        torch.cuda.synchronize()
        out.append(eng.global_flat.clone())
    assert torch.equal(out[0], out[1])
