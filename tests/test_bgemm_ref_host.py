"""Host-side checks behind the batched-GEMM and row-sum tests (no GPU): the
references of tests/bgemm_ref.py against fp64, and the argument checks and
workspace sizes of flr_bgemm[_ex] / flr_sum_rows[_ex], which return before any
launch."""
import numpy as np
import torch

import bgemm_ref
from flr import _capi

ARG, UNSUP = _capi.FLR_ERR_ARG, _capi.FLR_ERR_UNSUPPORTED
P1, P2, P3, P4 = 0x10000, 0x20000, 0x30000, 0x40000  # dummy non-null "device" pointers, never dereferenced


# ---- the references -------------------------------------------------------
def test_int_reference_is_exact_at_the_deepest_shape():
    K, M, N, R = 1, 64, 40, 16400
    o = bgemm_ref.int_operands(K, M, N, R)
    ref64 = torch.bmm(o["A"].double(), o["B"].double().transpose(1, 2))
    assert torch.equal(o["ref"].double(), ref64)
    # every value stored is what the kernels will read, and it is exact in fp32
    assert torch.equal(o["ref"].float().long(), o["ref"])
    assert o["A"].abs().max() == 3 and o["B"].abs().max() == 3 and o["bias"].abs().max() == 8
    assert sorted(o["mask"].unique().tolist()) == [0.0, 2.0]
    pre, out = bgemm_ref.int_epilogue(o, bias=True, add=True, act="relu", mask=True)
    want = (ref64 + o["bias"].double().unsqueeze(1)) + o["add"].double()
    assert torch.equal(pre.double(), want)
    assert torch.equal(out.double(), want.clamp(min=0) * o["mask"].double())
    assert int(out.abs().max()) < 2 ** 25  # the doubled value: still an fp32 integer
    _, dr = bgemm_ref.int_epilogue(o, act="drelu")
    assert torch.equal(dr.double(), torch.where(o["aux"] > 0, ref64, torch.zeros_like(ref64)))
    assert (o["aux"] == 0).any() and (o["aux"] < 0).any()


def test_split_rule_at_its_thresholds():
    """The thresholds the rule implies for a one-tile product: S = 2 / 4 / 8 / 16 from
    R = 2017 / 4065 / 8161 / 16353 (64 / 128 / 256 / 512 K-tiles, one more element
    than the K-tile count below)."""
    for S, R in ((2, 2017), (4, 4065), (8, 8161), (16, 16353)):
        assert bgemm_ref.splits(64, 64, R, 1) == S and bgemm_ref.splits(64, 64, R - 1, 1) == S // 2
    assert bgemm_ref.splits(64, 64, 1 << 20, 1) == 16
    # 16 tiles per client never split; 12 tiles split once (24 >= 16)
    assert bgemm_ref.splits(256, 256, 1 << 20, 1) == 1 and bgemm_ref.splits(130, 200, 1 << 20, 1) == 2
    assert bgemm_ref.tile(128, 128, 256) == 22 and bgemm_ref.tile(128, 128, 255) == 11
    assert bgemm_ref.tile(129, 257, 36) == 11 and bgemm_ref.tile(129, 513, 36) == 22
    assert bgemm_ref.tile(128, 512, 1) == 22 and bgemm_ref.tile(127, 999, 999) == 11
    assert bgemm_ref.grid(3, 70, 96, 130) == 12 and bgemm_ref.grid(2, 130, 200, 2080) == 16


def test_sum_rows_emulation_against_fp64():
    g = torch.Generator().manual_seed(1)
    for M in (1, 7, 9, 257, 513, 2080):
        X = torch.randn(2, M, 70, generator=g)
        ref = X.double().sum(dim=1)
        for chunked in (False, True):
            got = bgemm_ref.sum_rows_emulated(X, chunked)
            assert got.dtype == torch.float32 and got.shape == (2, 70)
            err = (got.double() - ref).abs().max().item()
            assert err <= 1e-6 * max(ref.abs().max().item(), 1.0), (M, chunked, err)
    # exact where fp32 is: integers, and the order of the rows
    X = torch.arange(2 * 21 * 3, dtype=torch.float32).reshape(2, 21, 3)
    assert torch.equal(bgemm_ref.sum_rows_emulated(X, False), X.sum(dim=1))


def test_sum_rows_orders_are_distinguishable():
    """At M = 513 the chunked and the one-pass order differ in bits, and both
    differ from a plain running sum: a kernel that took the other order fails a
    torch.equal comparison."""
    g = torch.Generator().manual_seed(2)
    X = torch.randn(2, 513, 70, generator=g)
    one, chunked = bgemm_ref.sum_rows_emulated(X, False), bgemm_ref.sum_rows_emulated(X, True)
    assert not torch.equal(one, chunked)
    seq = np.zeros((2, 70), np.float32)
    for m in range(513):
        seq = seq + X[:, m].numpy()
    assert not np.array_equal(seq, one.numpy()) and not np.array_equal(seq, chunked.numpy())
    # up to 256 rows, and past 64 chunks, there is one order only
    for M in (256, 64 * 256 + 1):
        Y = torch.randn(1, M, 3, generator=g)
        assert torch.equal(bgemm_ref.sum_rows_emulated(Y, False), bgemm_ref.sum_rows_emulated(Y, True))


# ---- argument validation: every call returns before any launch --------------
def _ex(**kw):
    a = dict(A=P1, a_k=64 * 32, a_m=32, a_r=1, B=P2, b_k=48 * 32, b_n=32, b_r=1, C=P3, c_k=64 * 48, c_m=48, c_n=1,
             bias=None, bias_k=0, add=None, act=0, mul=None, aux=None, pre=None, batch=2, M=64, N=48, R=32, ws=None,
             ws_bytes=0)
    a.update(kw)
    return _capi.lib().flr_bgemm_ex(
        a["A"], a["a_k"], a["a_m"], a["a_r"], a["B"], a["b_k"], a["b_n"], a["b_r"], a["C"], a["c_k"], a["c_m"],
        a["c_n"], a["bias"], a["bias_k"], a["add"], a["act"], a["mul"], a["aux"], a["pre"], a["batch"], a["M"],
        a["N"], a["R"], a["ws"], a["ws_bytes"], None)


def test_bgemm_ex_argument_validation_without_gpu():
    assert _ex(A=None) == ARG and _ex(B=None) == ARG and _ex(C=None) == ARG
    assert _ex(batch=0) == ARG and _ex(batch=-1) == ARG and _ex(batch=65536) == ARG
    assert _ex(M=0) == ARG and _ex(N=0) == ARG and _ex(R=0) == ARG
    for s in ("a_k", "a_m", "a_r", "b_k", "b_n", "b_r", "c_k", "c_m", "c_n"):
        assert _ex(**{s: -1}) == ARG, s
    assert _ex(act=-1) == ARG and _ex(act=7) == ARG
    for act in (4, 5, 6):  # DRELU, DGELU, DTANH read aux
        assert _ex(act=act) == ARG, act
        assert _ex(act=act, mul=P4, pre=P4) == ARG, act
    # an operand whose last element lies 2^29 floats (2^31 bytes) from its base: past the buffer offsets
    lim = 1 << 29
    assert _ex(M=2, a_m=lim - 32) == UNSUP          # (M-1) a_m + (R-1) a_r + 1 = 2^29
    assert _ex(N=2, b_n=lim - 32) == UNSUP
    assert _ex(R=2, a_r=lim - 63 * 32 - 1) == UNSUP
    # M N = 2^31 output elements per client (operands of one element: strides 0)
    assert _ex(M=1 << 16, N=1 << 15, R=1, a_m=0, b_n=0) == UNSUP
    # flr_bgemm is the same entry without an epilogue
    f = _capi.lib().flr_bgemm
    good = [P1, 64 * 32, 32, 1, P2, 48 * 32, 32, 1, P3, 64 * 48, 48, 1, None, 0, None, 2, 64, 48, 32, None, 0, None]
    for i in (0, 4, 8):
        a = list(good)
        a[i] = None
        assert f(*a) == ARG, i
    for i in (15, 16, 17, 18):
        a = list(good)
        a[i] = 0
        assert f(*a) == ARG, i


def test_sum_rows_argument_validation_without_gpu():
    f = _capi.lib().flr_sum_rows_ex  # (X, x_k, x_m, batch, M, N, out, out_k, ws, ws_bytes, stream)
    assert f(None, 64, 8, 2, 8, 8, P2, 8, None, 0, None) == ARG
    assert f(P1, 64, 8, 2, 8, 8, None, 8, None, 0, None) == ARG
    assert f(P1, 64, 8, 0, 8, 8, P2, 8, None, 0, None) == ARG
    assert f(P1, 64, 8, 65536, 8, 8, P2, 8, None, 0, None) == ARG
    assert f(P1, 64, 8, 2, 8, 0, P2, 8, None, 0, None) == ARG
    assert f(P1, 64, 8, 2, -1, 8, P2, 8, None, 0, None) == ARG
    g = _capi.lib().flr_sum_rows     # the same without a workspace
    assert g(None, 64, 8, 2, 8, 8, P2, 8, None) == ARG and g(P1, 64, 8, 2, 8, 8, None, 8, None) == ARG
    assert g(P1, 64, 8, 0, 8, 8, P2, 8, None) == ARG and g(P1, 64, 8, 2, 8, 0, P2, 8, None) == ARG
    assert g(P1, 64, 8, 2, -1, 8, P2, 8, None) == ARG


# ---- workspace sizes at hand-derived points ----------------------------------
def test_bgemm_workspace_sizes():
    ws = _capi.lib().flr_bgemm_workspace
    assert ws(1, 64, 64, 2048) == 2 * 64 * 64 * 4 == 32768          # 64 K-tiles: S = 2
    assert ws(1, 64, 64, 16384) == 16 * 64 * 64 * 4 == 262144       # 512 K-tiles: S = 16
    # 256 K-tiles; four 64 x 64 tiles split 4 ways (16 tiles), one 128 x 128 tile 8 ways: the larger
    assert ws(1, 128, 128, 8192) == 8 * 128 * 128 * 4 == 524288
    assert ws(3, 32, 256, 768) == 0                                 # 24 K-tiles: never split
    assert ws(0, 64, 64, 2048) == 0
    assert ws(2, 64, 64, 2016) == 0 and ws(2, 64, 64, 2017) == 2 * 2 * 64 * 64 * 4
    for K, M, N, R in ((2, 130, 200, 2080), (1, 33, 64, 8192), (1, 64, 40, 16400), (2, 60, 68, 2080),
                       (1, 64, 64, 4100), (3, 70, 96, 130)):
        assert ws(K, M, N, R) == bgemm_ref.workspace_bytes(K, M, N, R), (K, M, N, R)


def test_sum_rows_workspace_sizes():
    ws = _capi.lib().flr_sum_rows_workspace
    assert ws(2, 256, 70) == 0
    assert ws(2, 257, 70) == 1280                    # align_up(2 clients * 2 chunks * 70 * 4 = 1120, 256)
    assert ws(2, 16384, 70) == 2 * 64 * 70 * 4       # 64 chunks: 35840, a multiple of 256
    assert ws(2, 16385, 70) == 2 * 64 * 70 * 4       # 65 chunks: the 64-chunk size (the call runs one pass)
    assert ws(0, 513, 70) == 0 and ws(2, 513, 0) == 0
    for K, M, N in ((2, 513, 1), (2, 2080, 257), (5, 513, 70)):
        assert ws(K, M, N) == bgemm_ref.sum_rows_workspace_bytes(K, M, N)
