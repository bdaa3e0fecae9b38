"""Every path of the encoder kernels of csrc/train_xfmr.hip at the sizes where
they branch, against tests/xfmr_ref.py (test_xfmr_ref_host.py pins that to
torch): attention at every tile count NT = ceil(T / 16) in both thread forms
and every T mod 4, softmax inputs far from N(0, 1), the embedding sort at two
pairs per thread and its scatter past 256 columns, the uint32 sort key at its
limit, the out-of-range-id and zero_fill contracts, LayerNorm at one lane,
partial lane groups, row strides and the LN_CHUNK edge, flr_fill's unaligned
and tail paths, flr_vit_tokens, and "a client's result never depends on the
launch it shares".

Outputs of the direct C calls live inside larger device allocations with
GUARD sentinel floats on both sides and start as a NaN pattern: a call must
write all of its output and nothing else.

Bounds.  On randn inputs the project's own: 2e-6 forward (and lse, mean, rstd),
1e-5 backward, per slice (xfmr_ref.rel_by_slice: per head and per dq / dk / dv
for attention, per tensor for LayerNorm).  Where the inputs are built to be
hard (FP32_ERR, LN_HARD_FP32_ERR) the bound is MARGIN x the error of the same
formulas evaluated in fp32 by torch on the CPU against their fp64 evaluation at
these seeded inputs; _measure_fp32() prints those figures again and needs no GPU
(PYTHONPATH=multimodal-fl-security_amd:tests
python -c "import test_gpu_xfmr_edges as t; t._measure_fp32()")."""
import functools
import math

import pytest
import torch

import xfmr_ref
from xfmr_ref import WHOLE, head_slices, rel_by_slice
from flr import _capi
from flr import nn as fnn

pytestmark = pytest.mark.gpu

DH = 64
GUARD = 256
GUARD_BITS = 0x7FCA11CE  # quiet NaNs with payloads: nothing computes these
NAN_BITS = 0x7FC5A5A5
FWD_TOL, BWD_TOL = 2e-6, 1e-5
MARGIN = 8
U = 2.0 ** -24
FORMS = (None, "256", "512")  # FLR_ATT_THREADS: the default choice, and each form forced
ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = _capi.FLR_ERR_ARG, _capi.FLR_ERR_UNSUPPORTED, _capi.FLR_ERR_WORKSPACE


def bits(t):
    return t.contiguous().view(torch.int32)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _report(what, figures, bound):
    print(f"  {what}: " + " ".join(f"{k}={v:.3g}" for k, v in figures.items()) + f"  (bound {bound})")


class Guarded:
    """n floats inside a device allocation, GUARD (+ lead) sentinel floats
    before and GUARD after; the floats hold ``init`` or the NaN pattern."""

    def __init__(self, dev, n, init=None, lead=0):
        self.n, self.lo = n, GUARD + lead
        self.buf = torch.full((self.lo + n + GUARD,), GUARD_BITS, dtype=torch.int32, device=dev)
        if init is None:
            self.buf[self.lo:self.lo + n] = NAN_BITS
        else:
            self.buf[self.lo:self.lo + n] = bits(init).reshape(-1).to(dev)

    @property
    def t(self):
        return self.buf[self.lo:self.lo + self.n].view(torch.float32)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.lo

    def intact(self):
        return bool((self.buf[:self.lo] == GUARD_BITS).all() and (self.buf[self.lo + self.n:] == GUARD_BITS).all())

    def untouched(self):
        return self.intact() and bool((self.buf[self.lo:self.lo + self.n] == NAN_BITS).all())


class Rows:
    """A rows x D matrix at row stride ld inside rows * ldmax floats (so a row
    stride taken from another operand of the call stays inside), guards on both
    sides; the pad columns and the tail hold the sentinel.  read() checks that
    everything outside the matrix kept its bits and returns the matrix."""

    def __init__(self, dev, rows, D, ld, ldmax, init=None):
        self.shape, self.ld = (rows, D), ld
        self.before = torch.full((GUARD + rows * ldmax + GUARD,), GUARD_BITS, dtype=torch.int32)
        self.idx = (GUARD + torch.arange(rows)[:, None] * ld + torch.arange(D)[None, :]).reshape(-1)
        self.before[self.idx] = NAN_BITS if init is None else bits(init).reshape(-1)
        self.buf = self.before.to(dev)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * GUARD

    def read(self):
        after = self.buf.cpu()
        outside = torch.ones(after.numel(), dtype=torch.bool)
        outside[self.idx] = False
        assert torch.equal(after[outside], self.before[outside]), "wrote outside its rows"
        return after[self.idx].view(torch.float32).reshape(self.shape)


# ---------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------
ATT_T = [1, 2, 3, 4, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 95, 96]
SHIFT = 32.0


def _att(qkv, dctx, H):
    """flr_attention_fwd / _bwd on device qkv [KB, T, 3D], dctx [KB, T, D] ->
    ctx [KB, T, D], lse [KB, H, T], dqkv [KB, T, 3D]; the guards are checked."""
    KB, T, D3 = qkv.shape
    dev = qkv.device
    ctx, lse, dqkv = Guarded(dev, KB * T * D3 // 3), Guarded(dev, KB * H * T), Guarded(dev, KB * T * D3)
    _capi.call("flr_attention_fwd", qkv.data_ptr(), KB, T, H, DH, ctx.ptr, lse.ptr, _stream(dev))
    _capi.call("flr_attention_bwd", qkv.data_ptr(), ctx.ptr, dctx.data_ptr(), lse.ptr, KB, T, H, DH, dqkv.ptr,
               _stream(dev))
    assert ctx.intact() and lse.intact() and dqkv.intact()
    return ctx.t.view(KB, T, D3 // 3), lse.t.view(KB, H, T), dqkv.t.view(KB, T, D3)


def _att_inputs(T, H, case):
    """K = 2 clients x B = 2 rows (KB = 4), every (sequence, head) its own data."""
    D = H * DH
    g = torch.Generator().manual_seed(1000 * T + H)
    qkv = torch.randn(4, T, 3 * D, generator=g)
    dctx = torch.randn(4, T, D, generator=g)
    if case == "scaled":    # scores of std ~ 36: expf overflows without the row maximum
        qkv[..., :2 * D] *= 6
    elif case == "qshift":  # head 1's q + c: score (i, j) moves by c sum_d k[j][d] / 8
        qkv[..., DH:2 * DH] += SHIFT
    elif case == "kshift":  # head 1's k + c: row i's scores all move by c sum_d q[i][d] / 8 (P unchanged, lse moves)
        qkv[..., D + DH:D + 2 * DH] += SHIFT
    elif case == "qzero":
        qkv[..., :D] = 0
    else:
        assert case == "randn"
    return qkv, dctx


def _att_eval(qkv, dctx, H, dtype):
    ctx, lse = xfmr_ref.attention_ref(qkv, H, dtype)
    return ctx, lse, torch.cat(xfmr_ref.attention_bwd_ref(qkv, dctx, H, dtype), -1)


@functools.lru_cache(maxsize=None)
def _att_problem(T, H, case="randn"):
    qkv, dctx = _att_inputs(T, H, case)
    return (qkv, dctx) + _att_eval(qkv, dctx, H, torch.float64)


def _att_errors(got, ref, H):
    """rel_by_slice per head of ctx, lse and of dq, dk, dv."""
    per_head = head_slices(H, DH, 3)
    out = {"ctx": rel_by_slice(got[0], ref[0], head_slices(H, DH)),
           "lse": rel_by_slice(got[1], ref[1], [(slice(None), h) for h in range(H)])}
    for i, name in enumerate(("dq", "dk", "dv")):
        out[name] = rel_by_slice(got[2], ref[2], per_head[i * H:(i + 1) * H])
    return out


def _att_forms(cuda, knob, T, H, case):
    """The problem run in each thread form: [(ctx, lse, dqkv)] for FORMS, all
    finite, the two forced forms bit-identical."""
    qkv, dctx = (t.to(cuda) for t in _att_problem(T, H, case)[:2])
    outs = []
    for form in FORMS:
        knob("FLR_ATT_THREADS", form)
        outs.append(_att(qkv, dctx, H))
        assert all(bool(torch.isfinite(t).all()) for t in outs[-1]), form
    for a, b in zip(outs[1], outs[2]):
        assert torch.equal(bits(a), bits(b))
    assert any(all(torch.equal(bits(a), bits(b)) for a, b in zip(outs[0], o)) for o in outs[1:])
    return outs


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("T", ATT_T)
def test_attention_every_tile_count_and_form(cuda, knob, T, H):
    """NT = 1..6 x {256, 512} threads (and the default's choice between them),
    every T mod 4, both sides of each switch: ctx, lse, dq, dk, dv per head."""
    ref = _att_problem(T, H)
    for form, got in zip(FORMS, _att_forms(cuda, knob, T, H, "randn")):
        e = _att_errors(got, ref[2:], H)
        _report(f"T={T} H={H} form={form}", e, "2e-6 fwd / 1e-5 bwd")
        assert e["ctx"] < FWD_TOL and e["lse"] < FWD_TOL, (form, e)
        assert e["dv"] < BWD_TOL, (form, e)
        assert rel_by_slice(got[2], ref[4], WHOLE) < BWD_TOL  # the bound as it stood: dq | dk | dv together
        if T > 1:
            assert e["dq"] < BWD_TOL and e["dk"] < BWD_TOL, (form, e)
        else:
            _check_single_token_grads(got[2].cpu(), ref[0], ref[1], H)


def _check_single_token_grads(dqkv, qkv, dctx, H):
    """T = 1: P = 1 whatever q and k are, so dq = dk = 0 exactly and an error
    relative to them means nothing.  What the kernel computes is
    dS = (dP - Drow) / 8 with dP and Drow two fp32 sums of the same 64 products
    dO[d] v[d] in different orders (O = v exactly), each within 65 u sum|dO v|
    of the true sum, then dq[e] = dS k[e] and dk[e] = dS q[e] with one rounding:
    |dq[e]| <= 2 * 66 u * sum_d |dO[d] v[d]| / 8 * |k[e]|, and dk with q."""
    D = H * DH
    q, k, v = (xfmr_ref._heads(qkv[..., i * D:(i + 1) * D].double(), H) for i in range(3))
    a = (xfmr_ref._heads(dctx.double(), H) * v).abs().sum(-1, keepdim=True)
    c = 2 * 66 * U / 8
    dq, dk = (xfmr_ref._heads(dqkv[..., i * D:(i + 1) * D].double(), H) for i in range(2))
    assert bool((dq.abs() <= c * a * k.abs()).all()) and bool((dk.abs() <= c * a * q.abs()).all())
    assert torch.equal(dqkv[..., 2 * D:], dctx)  # dV = P^T dO = dO


# rel_by_slice of xfmr_ref evaluated in fp32 by torch on the CPU against its
# fp64 evaluation, at _att_inputs(T, 3, case): (ctx, lse, dq, dk, dv).  The
# test allows MARGIN = 8 x each figure: the kernels' fma chains sum in another
# order than torch's GEMM, and an fp32 dot product's error depends on the order
# by about that factor.
FP32_ERR = {
    "scaled": {17: (5.8e-06, 2.2e-07, 3.4e-06, 4.9e-06, 1.6e-06),   # bounds 4.6e-5 1.8e-6 2.7e-5 3.9e-5 1.3e-5
               64: (5.8e-06, 2.6e-07, 1.2e-05, 1.3e-05, 3.1e-06),   # 4.6e-5 2.1e-6 9.6e-5 1.0e-4 2.5e-5
               96: (6.9e-06, 2.5e-07, 1.3e-05, 1.8e-05, 4.1e-06)},  # 5.5e-5 2.0e-6 1.0e-4 1.4e-4 3.3e-5
    "qshift": {17: (4.7e-06, 2.2e-07, 3.8e-06, 3.7e-06, 2.8e-06),   # 3.8e-5 1.8e-6 3.0e-5 3.0e-5 2.2e-5
               64: (5.4e-06, 2.5e-07, 4.2e-06, 2.4e-06, 7.1e-07),   # 4.3e-5 2.0e-6 3.4e-5 1.9e-5 5.7e-6
               96: (5.9e-06, 4.3e-07, 2.0e-05, 4.0e-05, 6.1e-07)},  # 4.7e-5 3.4e-6 1.6e-4 3.2e-4 4.9e-6
    "kshift": {17: (5.4e-06, 1.2e-07, 4.9e-06, 4.2e-06, 3.5e-06),   # 4.3e-5 9.6e-7 3.9e-5 3.4e-5 2.8e-5
               64: (8.3e-06, 9.0e-08, 5.4e-06, 6.2e-06, 5.5e-06),   # 6.6e-5 7.2e-7 4.3e-5 5.0e-5 4.4e-5
               96: (8.6e-06, 8.9e-08, 7.7e-06, 5.6e-06, 5.1e-06)},  # 6.9e-5 7.1e-7 6.2e-5 4.5e-5 4.1e-5
}
RANGE_T = [17, 64, 96]
QTY = ("ctx", "lse", "dq", "dk", "dv")


@pytest.mark.parametrize("T", RANGE_T)
@pytest.mark.parametrize("case", list(FP32_ERR))
def test_attention_softmax_range(cuda, knob, case, T):
    """Scores far from N(0, 1): q and k scaled by 6 (row maxima past expf's
    overflow at 88.7), one head's q + 32 (scores of that head move by
    32 sum_d k[j][d] / 8, column by column), one head's k + 32 (row i's scores
    all move by 32 sum_d q[i][d] / 8: softmax is invariant, lse is not).  Wrong
    without the row-maximum subtraction, or with lse off by a constant."""
    H = 3
    ref = _att_problem(T, H, case)
    assert ref[3].abs().max() > 50  # the case is what it says: lse far outside randn's few units
    bound = dict(zip(QTY, (MARGIN * f for f in FP32_ERR[case][T])))
    for form, got in zip(FORMS, _att_forms(cuda, knob, T, H, case)):
        e = _att_errors(got, ref[2:], H)
        _report(f"{case} T={T} form={form}", e, bound)
        for name in QTY:
            assert e[name] < bound[name], (form, name, e[name], bound[name])


@pytest.mark.parametrize("T", RANGE_T)
def test_attention_uniform_softmax(cuda, knob, T):
    """q = 0: every score is 0, P = 1 / T.  ctx rows are the mean of v and
    lse = log T (1e-6, straight from v); dk = dS^T Q = 0 exactly;
    dV[j] = (1 / T) sum_i dO[i]; dQ[i] = (1 / 8T) sum_j (dO[i] . (v[j] - mean v)) k[j]
    (not 0: k is not) -- both written out here in fp64, without the reference."""
    H, D = 3, 3 * DH
    qkv, dctx = _att_problem(T, H, "qzero")[:2]
    k, v = (xfmr_ref._heads(qkv[..., i * D:(i + 1) * D].double(), H) for i in (1, 2))
    do = xfmr_ref._heads(dctx.double(), H)
    vbar = v.mean(-2, keepdim=True)
    want_ctx = xfmr_ref._merge(vbar.expand_as(v))
    want_dv = xfmr_ref._merge(do.mean(-2, keepdim=True).expand_as(v))
    want_dq = xfmr_ref._merge((do @ (v - vbar).transpose(-2, -1)) @ k / (8 * T))
    per_head = head_slices(H, DH)
    for form, (ctx, lse, dqkv) in zip(FORMS, _att_forms(cuda, knob, T, H, "qzero")):
        e = {"ctx": rel_by_slice(ctx, want_ctx, per_head),
             "lse": ((lse.double().cpu() - math.log(T)).abs().max() / math.log(T)).item(),
             "dq": rel_by_slice(dqkv[..., :D], want_dq, per_head),
             "dv": rel_by_slice(dqkv[..., 2 * D:], want_dv, per_head)}
        _report(f"q=0 T={T} form={form}", e, "1e-6 fwd / 1e-5 bwd")
        assert e["ctx"] < 1e-6 and e["lse"] < 1e-6, (form, e)
        assert bool((dqkv[..., D:2 * D] == 0).all()), form
        assert e["dq"] < BWD_TOL and e["dv"] < BWD_TOL, (form, e)


@pytest.mark.parametrize("form", ["256", "512"])
@pytest.mark.parametrize("T", [1, 5, 65, 81, 96])
def test_attention_writes_all_of_its_outputs_and_nothing_else(cuda, knob, T, form):
    """ctx, lse and dqkv start as NaN between sentinel guards (_att): every
    element is written (dqkv is overwritten, not accumulated into), rows >= T of
    the last sequence (the 16-row tiles' overhang) are not."""
    knob("FLR_ATT_THREADS", form)
    qkv, dctx = (t.to(cuda) for t in _att_problem(T, 3)[:2])
    for t in _att(qkv, dctx, 3):
        assert bool(torch.isfinite(t).all())


def test_attention_rejects_what_it_cannot_run(cuda):
    """Another head width or T > 96: FLR_ERR_UNSUPPORTED; no sequences or no
    tokens: FLR_ERR_ARG; nothing is launched (the outputs keep their prefill)."""
    lib, st = _capi.lib(), _stream(cuda)
    qkv = torch.randn(2, 97, 3 * DH, device=cuda)
    ctx, lse, dqkv = Guarded(cuda, 2 * 97 * DH), Guarded(cuda, 2 * 97), Guarded(cuda, 2 * 97 * 3 * DH)
    dctx = torch.randn(2, 97, DH, device=cuda)
    for KB, T, dh, want in ((2, 16, 32, ERR_UNSUPPORTED), (2, 97, DH, ERR_UNSUPPORTED), (0, 16, DH, ERR_ARG),
                            (2, 0, DH, ERR_ARG)):
        assert lib.flr_attention_fwd(qkv.data_ptr(), KB, T, 1, dh, ctx.ptr, lse.ptr, st) == want
        assert lib.flr_attention_bwd(qkv.data_ptr(), qkv.data_ptr(), dctx.data_ptr(), qkv.data_ptr(), KB, T, 1, dh,
                                     dqkv.ptr, st) == want
    torch.cuda.synchronize()
    assert ctx.untouched() and lse.untouched() and dqkv.untouched()


@pytest.mark.parametrize("T", [5, 64, 65, 96])
def test_attention_sequences_and_heads_are_independent(cuda, T):
    """A (sequence, head)'s ctx, lse and gradients out of a KB = 6, H = 3 launch
    are the bits of that sequence run alone (KB = 1) and of that head run alone
    (qkv sliced into an H = 1 problem)."""
    KB, H, D = 6, 3, 3 * DH
    g = torch.Generator().manual_seed(T)
    qkv = torch.randn(KB, T, 3 * D, generator=g).to(cuda)
    dctx = torch.randn(KB, T, D, generator=g).to(cuda)
    ctx, lse, dqkv = _att(qkv, dctx, H)
    for kb in range(KB):
        one = _att(qkv[kb:kb + 1].contiguous(), dctx[kb:kb + 1].contiguous(), H)
        for a, b in zip(one, (ctx, lse, dqkv)):
            assert torch.equal(bits(a[0]), bits(b[kb])), kb
    for h in range(H):
        col = slice(h * DH, (h + 1) * DH)
        q1 = torch.cat([qkv[..., i * D:(i + 1) * D][..., col] for i in range(3)], -1).contiguous()
        c1, l1, d1 = _att(q1, dctx[..., col].contiguous(), 1)
        assert torch.equal(bits(c1), bits(ctx[..., col])) and torch.equal(bits(l1[:, 0]), bits(lse[:, h]))
        for i in range(3):
            assert torch.equal(bits(d1[..., i * DH:(i + 1) * DH]), bits(dqkv[..., i * D:(i + 1) * D][..., col])), (h, i)


# ---------------------------------------------------------------------------
# embedding
# ---------------------------------------------------------------------------
EMB_SHAPES = [  # (K, V, E, N)
    (1, 11, 4, 1),
    (2, 97, 12, 2049),     # NP = 4096: two pairs per thread and stage, 2047 padding keys
    (2, 500, 64, 3072),    # the workload's N = 32 * 96
    (1, 3000, 260, 4096),  # NP = N = SORT_MAX; second trip of the scatter's column loop, 4 of 256 columns
    (2, 40, 320, 1000),    # second trip with one full lane group
    (1, 9, 516, 33),       # third trip
]


def _emb_ids(pattern, K, V, N, g):
    if pattern == "distinct":
        return torch.stack([torch.randperm(V, generator=g)[:N] for _ in range(K)])
    ids = torch.randint(0, V, (K, N), generator=g)
    n = N // 4 if pattern == "quarter" else N
    ids[:, :n] = ids[:, :1]  # one id over a long run of positions
    return ids


def _emb_check(cuda, table, ids, dout):
    """client_embedding forward and backward, bit for bit."""
    K, V, E = table.shape
    t = table.to(cuda).requires_grad_(True)
    out = fnn.client_embedding(t, ids.to(cuda))
    (dt,) = torch.autograd.grad(out, t, dout.to(cuda))
    out, dt = out.cpu(), dt.cpu()
    for k in range(K):
        assert torch.equal(bits(out[k]), bits(table[k][ids[k]])), k
        assert torch.equal(bits(dt[k]), bits(xfmr_ref.embedding_bwd_ref(ids[k], dout[k], V))), k


EMB_CASES = [(s, p) for s in EMB_SHAPES for p in ("quarter", "same", "distinct")
             if p != "distinct" or s[1] >= s[3]]  # N distinct ids need V >= N


@pytest.mark.parametrize("shape,pattern", EMB_CASES, ids=[f"{s}-{p}".replace(" ", "") for s, p in EMB_CASES])
def test_embedding_sort_and_scatter_sizes(cuda, shape, pattern):
    K, V, E, N = shape
    g = torch.Generator().manual_seed(V + N)
    table = torch.randn(K, V, E, generator=g)
    _emb_check(cuda, table, _emb_ids(pattern, K, V, N, g), torch.randn(K, N, E, generator=g))


def test_embedding_sort_key_at_the_uint32_limit(cuda):
    """The key id * N + n with (V + 1) * N = 2^32 - 4096, the largest the
    entry accepts: ids 0, V - 1, V - 2, a run of V - 1, the rest random."""
    V, N, E = 1048574, 4096, 4
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(0, V, (1, N), generator=g)
    ids[0, :3] = torch.tensor([0, V - 1, V - 2])
    ids[0, 2000:2010] = V - 1
    ids[0, N - 1] = V - 1  # key (V - 1) * N + N - 1: the largest of all
    _emb_check(cuda, torch.randn(1, V, E, generator=g), ids, torch.randn(1, N, E, generator=g))


@pytest.mark.parametrize("V,N", [(1048575, 4096), (9, 4097)])
def test_embedding_bwd_rejects_keys_past_uint32_and_long_sorts(cuda, V, N):
    E = 4
    dout, ids = torch.zeros(N, E, device=cuda), torch.zeros(N, dtype=torch.int64, device=cuda)
    dtab = Guarded(cuda, V * E)
    n = int(_capi.lib().flr_embedding_bwd_workspace(1, N))
    ws = torch.empty(n, dtype=torch.uint8, device=cuda)
    rc = _capi.lib().flr_embedding_bwd(dout.data_ptr(), ids.data_ptr(), N, 1, N, V, E, dtab.ptr, V * E, 1,
                                       ws.data_ptr(), n, _stream(cuda))
    torch.cuda.synchronize()
    assert rc == ERR_UNSUPPORTED and dtab.untouched()


SPARE = 777.0


def _spared(table):
    """[K, V, E] -> [K, V + 2, E] with a spare row before and after each
    client's table: an index of -1 or V stays inside the allocation."""
    K, V, E = table.shape
    t = torch.full((K, V + 2, E), SPARE)
    t[:, 1:V + 1] = table
    return t


def _emb_bwd(cuda, dout, ids, ids_k, V, dtab, dtab_k, zero_fill, lead):
    """flr_embedding_bwd into the Guarded dtab, tables starting `lead` floats in."""
    K, N, E = dout.shape
    n = int(_capi.lib().flr_embedding_bwd_workspace(K, N))
    ws = torch.empty(n, dtype=torch.uint8, device=cuda)
    d, i = dout.to(cuda), ids.to(cuda)
    _capi.call("flr_embedding_bwd", d.data_ptr(), i.data_ptr(), ids_k, K, N, V, E, dtab.ptr + 4 * lead, dtab_k,
               zero_fill, ws.data_ptr(), n, _stream(cuda))
    torch.cuda.synchronize()
    assert dtab.intact()
    return dtab.t.cpu()


def test_embedding_out_of_range_ids(cuda):
    """include/flr.h: an id outside [0, V) yields a NaN row in the forward and
    is skipped by the backward; nothing is read or written outside the table.
    Each table has a spare row on both sides, so -1 and V would stay inside."""
    K, V, E, N = 2, 20, 12, 40
    g = torch.Generator().manual_seed(4)
    table = torch.randn(K, V, E, generator=g)
    ids = torch.randint(0, V, (K, N), generator=g)
    bad = {0: [0, 7, 39], 1: [13, 14]}
    for k, pos in bad.items():
        ids[k, pos] = torch.tensor([-1, V, -1])[:len(pos)]
    w = Guarded(cuda, K * (V + 2) * E, _spared(table))
    out = Guarded(cuda, K * N * E)
    idv = ids.to(cuda)
    _capi.call("flr_embedding_fwd", w.ptr + 4 * E, (V + 2) * E, V, idv.data_ptr(), N, None, 0, 0, None, 0, None, 0, 0,
               None, 0, K, N, E, out.ptr, _stream(cuda))
    torch.cuda.synchronize()
    got = out.t.cpu().view(K, N, E)
    assert out.intact()
    for k in range(K):
        for n in range(N):
            if n in bad[k]:
                assert bool(torch.isnan(got[k, n]).all()), (k, n)
            else:
                assert torch.equal(bits(got[k, n]), bits(table[k, ids[k, n]])), (k, n)
    # backward: the bad positions contribute nothing; spare rows, guards untouched
    dout = torch.randn(K, N, E, generator=g)
    dtab = Guarded(cuda, K * (V + 2) * E, torch.full((K, V + 2, E), SPARE))
    d = _emb_bwd(cuda, dout, ids, N, V, dtab, (V + 2) * E, 1, E).view(K, V + 2, E)
    for k in range(K):
        keep = torch.tensor([n for n in range(N) if n not in bad[k]])
        assert torch.equal(bits(d[k, 1:V + 1]), bits(xfmr_ref.embedding_bwd_ref(ids[k, keep], dout[k, keep], V))), k
        assert bool((d[k, 0] == SPARE).all()) and bool((d[k, V + 1] == SPARE).all()), k


def test_embedding_sum_bad_id_in_one_table_poisons_the_row(cuda):
    """(w0[ids0] + w1[ids1]) + w2[ids2] with ids1 / ids2 shared by the clients:
    a bad id in table 1 alone makes the row NaN, the other rows are the sum in
    that order, bit for bit."""
    K, E, N, V0, V1, V2 = 2, 12, 24, 30, 2, 24
    g = torch.Generator().manual_seed(6)
    w0, w1, w2 = (torch.randn(K, v, E, generator=g) for v in (V0, V1, V2))
    ids0 = torch.randint(0, V0, (K, N), generator=g)
    ids1 = torch.randint(0, V1, (N,), generator=g)
    ids2 = torch.arange(N)
    ids1[5], ids1[9] = V1, -1
    tabs = [Guarded(cuda, K * (v + 2) * E, _spared(w)) for w, v in ((w0, V0), (w1, V1), (w2, V2))]
    i0, i1, i2 = ids0.to(cuda), ids1.to(cuda), ids2.to(cuda)
    out = Guarded(cuda, K * N * E)
    _capi.call("flr_embedding_fwd", tabs[0].ptr + 4 * E, (V0 + 2) * E, V0, i0.data_ptr(), N,
               tabs[1].ptr + 4 * E, (V1 + 2) * E, V1, i1.data_ptr(), 0,
               tabs[2].ptr + 4 * E, (V2 + 2) * E, V2, i2.data_ptr(), 0, K, N, E, out.ptr, _stream(cuda))
    torch.cuda.synchronize()
    got = out.t.cpu().view(K, N, E)
    assert out.intact()
    for k in range(K):
        for n in range(N):
            if n in (5, 9):
                assert bool(torch.isnan(got[k, n]).all()), (k, n)
            else:
                want = (w0[k, ids0[k, n]] + w1[k, ids1[n]]) + w2[k, ids2[n]]
                assert torch.equal(bits(got[k, n]), bits(want)), (k, n)


def test_embedding_bwd_without_zero_fill_overwrites_touched_rows_only(cuda):
    K, V, E, N = 2, 50, 8, 30
    g = torch.Generator().manual_seed(8)
    ids = torch.randint(0, V, (K, N), generator=g)
    ids[:, :6] = ids[:, :1]
    dout = torch.randn(K, N, E, generator=g)
    pattern = torch.randn(K, V, E, generator=g)
    d = _emb_bwd(cuda, dout, ids, N, V, Guarded(cuda, K * V * E, pattern), V * E, 0, 0).view(K, V, E)
    for k in range(K):
        touched = torch.zeros(V, dtype=torch.bool)
        touched[ids[k]] = True
        assert 0 < int(touched.sum()) < V
        want = torch.where(touched[:, None], xfmr_ref.embedding_bwd_ref(ids[k], dout[k], V), pattern[k])
        assert torch.equal(bits(d[k]), bits(want)), k


def test_embedding_bwd_strided_tables_zero_fill_keeps_the_gaps(cuda):
    """dtable_k = V * E + 8: the zero fill runs per client and the 8 floats
    between the clients' tables keep their bits."""
    K, V, E, N = 3, 21, 12, 17
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(0, V, (K, N), generator=g)
    dout = torch.randn(K, N, E, generator=g)
    step = V * E + 8
    d = _emb_bwd(cuda, dout, ids, N, V, Guarded(cuda, K * step, torch.full((K * step,), SPARE)), step, 1, 0)
    d = d.view(K, step)
    for k in range(K):
        assert torch.equal(bits(d[k, :V * E].view(V, E)), bits(xfmr_ref.embedding_bwd_ref(ids[k], dout[k], V))), k
        assert bool((d[k, V * E:] == SPARE).all()), k


def test_embedding_bwd_shared_ids_each_client_its_own_dout(cuda):
    K, V, E, N = 3, 15, 8, 64
    g = torch.Generator().manual_seed(10)
    ids = torch.randint(0, V, (N,), generator=g)
    dout = torch.randn(K, N, E, generator=g)
    d = _emb_bwd(cuda, dout, ids, 0, V, Guarded(cuda, K * V * E), V * E, 1, 0).view(K, V, E)
    for k in range(K):
        assert torch.equal(bits(d[k]), bits(xfmr_ref.embedding_bwd_ref(ids, dout[k], V))), k


# ---------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------
LN_K = 3
LN_CASES = [  # (D, rows_per_client, residual + dskip, eps): every D, every rows_per_client, every eps
    (4, 1, False, 1e-5),      # one lane; three clients' rows in one 4-wave block
    (4, 65, True, 1e-12),     # LN_CHUNK + 1: a second chunk of one row
    (8, 3, True, 1e-6),
    (8, 129, False, 1e-5),    # three chunks
    (252, 63, True, 1e-12),   # 63 lanes
    (252, 64, False, 1e-6),   # exactly one chunk
    (256, 64, True, 1e-5),
    (256, 1, True, 1e-12),
    (260, 65, False, 1e-6),   # a second lane group of one lane
    (260, 3, True, 1e-5),
    (1020, 129, True, 1e-12),  # last lane group one lane short
    (1020, 1, False, 1e-6),
    (1024, 63, False, 1e-5),
    (1024, 3, True, 1e-6),
]
LN_NAMES = ("y", "s", "mean", "rstd", "dx", "dgamma", "dbeta")


def _ln_inputs(D, R, res, hard=False):
    g = torch.Generator().manual_seed(1000 * D + R)
    rnd = lambda *s: torch.randn(*s, generator=g)
    x = 1000 + 0.01 * rnd(LN_K, R, D) if hard else rnd(LN_K, R, D) * 2 + 0.5
    return dict(x=x, r=rnd(LN_K, R, D) if res else None, gamma=1 + 0.1 * rnd(LN_K, D), beta=0.1 * rnd(LN_K, D),
                dy=rnd(LN_K, R, D), dskip=rnd(LN_K, R, D) if res else None)


def _ln_eval(p, eps, dtype):
    y, s, mean, rstd = xfmr_ref.layernorm_ref(p["x"], p["gamma"], p["beta"], eps, p["r"], dtype)
    dx, dg, db = xfmr_ref.layernorm_bwd_ref(p["dy"], s, p["gamma"], mean, rstd, p["dskip"], dtype)
    return dict(zip(LN_NAMES, (y, s, mean, rstd, dx, dg, db)))


def _ln(cuda, p, eps, ld=None):
    """flr_layernorm_fwd / _bwd on the inputs p through the C entries; ld maps an
    operand (x, r, y, s, dy, dskip, dx) to its row stride (default D).  Every
    operand's pads, tail and guards are checked."""
    ld = ld or {}
    K, R, D = p["x"].shape
    rows, ldmax = K * R, max([D] + list(ld.values()))
    mk = lambda name, init=None: Rows(cuda, rows, D, ld.get(name, D), ldmax,
                                      None if init is None else init.reshape(rows, D))
    res = p["r"] is not None
    x, r, y, s = mk("x", p["x"]), (mk("r", p["r"]) if res else None), mk("y"), (mk("s") if res else None)
    dy, dskip, dx = mk("dy", p["dy"]), (mk("dskip", p["dskip"]) if res else None), mk("dx")
    mean, rstd, dg, db = Guarded(cuda, rows), Guarded(cuda, rows), Guarded(cuda, K * D), Guarded(cuda, K * D)
    gam, bet = p["gamma"].to(cuda), p["beta"].to(cuda)
    st = _stream(cuda)
    opt = lambda m: (None, 0) if m is None else (m.ptr, m.ld)
    _capi.call("flr_layernorm_fwd", x.ptr, x.ld, *opt(r), gam.data_ptr(), bet.data_ptr(), y.ptr, y.ld, *opt(s),
               mean.ptr, rstd.ptr, rows, D, R, eps, st)
    n = int(_capi.lib().flr_layernorm_bwd_workspace(K, R, D))
    ws = torch.empty(n, dtype=torch.uint8, device=cuda)
    src = s if res else x
    _capi.call("flr_layernorm_bwd", dy.ptr, dy.ld, src.ptr, src.ld, gam.data_ptr(), mean.ptr, rstd.ptr, *opt(dskip),
               dx.ptr, dx.ld, dg.ptr, db.ptr, K, R, D, ws.data_ptr(), n, st)
    torch.cuda.synchronize()
    assert mean.intact() and rstd.intact() and dg.intact() and db.intact()
    for m in (x, r, dy, dskip):
        if m is not None:
            m.read()  # the inputs kept their bits too
    return dict(y=y.read().view(K, R, D), s=s.read().view(K, R, D) if res else p["x"],
                mean=mean.t.cpu().view(K, R), rstd=rstd.t.cpu().view(K, R), dx=dx.read().view(K, R, D),
                dgamma=dg.t.cpu().view(K, D), dbeta=db.t.cpu().view(K, D))


LN_TOL = dict(y=FWD_TOL, mean=FWD_TOL, rstd=FWD_TOL, dx=BWD_TOL, dgamma=BWD_TOL, dbeta=BWD_TOL)


@pytest.mark.parametrize("D,R,res,eps", LN_CASES)
def test_layernorm_lane_groups_chunks_and_eps(cuda, D, R, res, eps):
    p = _ln_inputs(D, R, res)
    got, ref = _ln(cuda, p, eps), _ln_eval(p, eps, torch.float64)
    if res:
        assert torch.equal(bits(got["s"]), bits(p["x"] + p["r"]))
    e = {name: rel_by_slice(got[name], ref[name], WHOLE) for name in LN_TOL}
    _report(f"D={D} R={R} res={res} eps={eps}", e, "2e-6 fwd / 1e-5 bwd")
    for name, tol in LN_TOL.items():
        assert bool(torch.isfinite(got[name]).all()) and e[name] < tol, (name, e[name])


@pytest.mark.parametrize("D,R,res", [(8, 3, True), (260, 65, True), (1024, 5, False), (4, 66, True)])
def test_layernorm_row_strides(cuda, D, R, res):
    """Every operand at a row stride of D + 4 or D + 12, neighbours in the
    argument list at different ones: the bits of the contiguous call; pad
    columns, tails and guards untouched (Rows.read)."""
    p = _ln_inputs(D, R, res)
    ld = dict(x=D + 4, r=D + 12, y=D + 12, s=D + 4, dy=D + 12, dskip=D + 4, dx=D + 12)
    got, want = _ln(cuda, p, 1e-6, ld), _ln(cuda, p, 1e-6)
    for name in LN_NAMES:
        assert torch.equal(bits(got[name]), bits(want[name])), name


def test_layernorm_rejects_what_it_cannot_run(cuda):
    """A row stride that is no multiple of 4: FLR_ERR_UNSUPPORTED; D > 1024 or
    D % 4: FLR_ERR_ARG; a short workspace: FLR_ERR_WORKSPACE.  Nothing runs."""
    lib, st = _capi.lib(), _stream(cuda)
    K, R = 2, 3
    big = torch.zeros(K * R * 1040, device=cuda)
    vec = torch.zeros(K * 1040, device=cuda)
    outs = [Guarded(cuda, K * R * 1040) for _ in range(2)] + [Guarded(cuda, K * 1040) for _ in range(4)]
    y, dx, mean, rstd, dg, db = outs
    n = int(lib.flr_layernorm_bwd_workspace(K, R, 1024))
    ws = torch.empty(n, dtype=torch.uint8, device=cuda)

    def fwd(D, ldx, ldr, ldy, lds):
        return lib.flr_layernorm_fwd(big.data_ptr(), ldx, big.data_ptr(), ldr, vec.data_ptr(), vec.data_ptr(), y.ptr,
                                     ldy, dx.ptr, lds, mean.ptr, rstd.ptr, K * R, D, R, 1e-6, st)

    def bwd(D, lddy, lds, ldk, lddx, nbytes):
        return lib.flr_layernorm_bwd(big.data_ptr(), lddy, big.data_ptr(), lds, vec.data_ptr(), vec.data_ptr(),
                                     vec.data_ptr(), big.data_ptr(), ldk, dx.ptr, lddx, dg.ptr, db.ptr, K, R, D,
                                     ws.data_ptr(), nbytes, st)

    for i in range(4):
        lds = [64] * 4
        lds[i] = 66
        assert fwd(64, *lds) == ERR_UNSUPPORTED and bwd(64, *lds, n) == ERR_UNSUPPORTED
    for D in (1028, 6, 0):
        assert fwd(D, 1040, 1040, 1040, 1040) == ERR_ARG and bwd(D, 1040, 1040, 1040, 1040, n) == ERR_ARG
    need = int(lib.flr_layernorm_bwd_workspace(K, R, 64))
    assert bwd(64, 64, 64, 64, 64, need - 1) == ERR_WORKSPACE
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs)


# rel_by_slice (per tensor) of xfmr_ref's LayerNorm evaluated in fp32 by torch
# on the CPU against its fp64 evaluation at _ln_inputs(1020, 5, False,
# hard=True), eps 1e-6: rows of mean 1000 and deviation 0.01, where the mean's
# own rounding (sums near 2^20: steps of 2^-4) is a percent of the deviation
# and a one-pass variance has no correct digit.  The test allows MARGIN = 8 x.
LN_HARD = (1020, 5, 1e-6)
LN_HARD_FP32_ERR = dict(y=2.5e-3, mean=8.7e-08, rstd=3.6e-05, dx=1.8e-4, dgamma=3.3e-3, dbeta=6.7e-08)
#                bounds: y 2.0e-2, mean 7.0e-7, rstd 2.9e-4, dx 1.4e-3, dgamma 2.6e-2, dbeta 5.4e-7


def test_layernorm_mean_far_above_deviation(cuda):
    D, R, eps = LN_HARD
    p = _ln_inputs(D, R, False, hard=True)
    got, ref = _ln(cuda, p, eps), _ln_eval(p, eps, torch.float64)
    e = {name: rel_by_slice(got[name], ref[name], WHOLE) for name in LN_TOL}
    bound = {name: MARGIN * LN_HARD_FP32_ERR[name] for name in LN_TOL}
    _report("x = 1000 + 0.01 randn", e, bound)
    for name in LN_TOL:
        assert bool(torch.isfinite(got[name]).all()) and e[name] < bound[name], (name, e[name], bound[name])


@pytest.mark.parametrize("D,R,res", [(260, 3, True), (64, 65, True), (1024, 1, False)])
def test_layernorm_clients_are_independent(cuda, D, R, res):
    """Client k out of a K = 3 launch (rows of several clients in one block at
    R < 4) has the bits of a K = 1 launch of that client: y, s, mean, rstd, dx
    and the dgamma / dbeta sums."""
    p = _ln_inputs(D, R, res)
    all_ = _ln(cuda, p, 1e-6)
    for k in range(LN_K):
        one = _ln(cuda, {n: (None if t is None else t[k:k + 1]) for n, t in p.items()}, 1e-6)
        for name in LN_NAMES:
            assert torch.equal(bits(one[name][0]), bits(all_[name][k])), (k, name)


# ---------------------------------------------------------------------------
# fill, vit_tokens
# ---------------------------------------------------------------------------
FILL_N = [0, 1, 3, 4, 5, 1023, 1024, 1025, 4 * 256 * 16384 + 7]  # the last: past the 16384-block grid cap


@pytest.mark.parametrize("value", [0.0, -0.0, 1.5])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_fill_alignment_tail_and_grid_cap(cuda, offset, value):
    """p at `offset` floats past a 16-byte boundary (0: the vector path and its
    n % 4 tail; 1..3: the scalar path): n floats hold the value's bits (-0.0
    its sign), the floats on both sides keep theirs."""
    want = int(torch.tensor([value]).view(torch.int32).item())
    for n in FILL_N:
        g = Guarded(cuda, n, lead=offset)
        assert g.ptr % 16 == 4 * offset
        rc = _capi.lib().flr_fill(g.ptr, n, value, _stream(cuda))
        torch.cuda.synchronize()
        assert rc == 0 and g.intact() and bool((g.buf[g.lo:g.lo + n] == want).all()), n


VIT_SHAPES = [(1, 1, 1, 4), (3, 2, 5, 12), (2, 3, 64, 384)]


@pytest.mark.parametrize("K,B,P,D", VIT_SHAPES)
def test_vit_tokens_shapes(cuda, K, B, P, D):
    g = torch.Generator().manual_seed(K + B + P + D)
    tok, cls, pos = torch.randn(K, B * P, D, generator=g), torch.randn(K, 1, 1, D, generator=g), \
        torch.randn(K, P + 1, D, generator=g)
    dx = torch.randn(K, B, P + 1, D, generator=g)
    leaves = [t.to(cuda).requires_grad_(True) for t in (tok, cls, pos)]
    x0 = fnn.client_vit_tokens(*leaves, B)
    dtok, dcls, dpos = torch.autograd.grad(x0, leaves, dx.to(cuda))
    want = torch.cat([cls.expand(K, B, 1, D), tok.view(K, B, P, D)], 2) + pos.view(K, 1, P + 1, D)
    assert torch.equal(bits(x0.cpu()), bits(want))
    assert torch.equal(bits(dtok.cpu()), bits(dx[:, :, 1:].reshape(K, B * P, D)))  # a copy
    assert rel_by_slice(dcls, dx[:, :, 0].double().sum(1).view(K, 1, 1, D), WHOLE) < 1e-6
    assert rel_by_slice(dpos, dx.double().sum(1), WHOLE) < 1e-6


def test_vit_tokens_rejects_a_width_that_is_no_multiple_of_4(cuda):
    t = torch.zeros(64, device=cuda)
    x0 = Guarded(cuda, 64)
    rc = _capi.lib().flr_vit_tokens(t.data_ptr(), t.data_ptr(), t.data_ptr(), 1, 1, 1, 6, x0.ptr, _stream(cuda))
    torch.cuda.synchronize()
    assert rc == ERR_ARG and x0.untouched()


def _measure_fp32():
    """The figures of FP32_ERR and LN_HARD_FP32_ERR: fp32 on the CPU against fp64."""
    for case in FP32_ERR:
        for T in RANGE_T:
            qkv, dctx = _att_inputs(T, 3, case)
            e = _att_errors(_att_eval(qkv, dctx, 3, torch.float32), _att_eval(qkv, dctx, 3, torch.float64), 3)
            print(f'FP32_ERR["{case}"][{T}] = (' + ", ".join(f"{e[q]:.2g}" for q in QTY) + ")")
    D, R, eps = LN_HARD
    p = _ln_inputs(D, R, False, hard=True)
    lo, hi = _ln_eval(p, eps, torch.float32), _ln_eval(p, eps, torch.float64)
    print("LN_HARD_FP32_ERR = dict(" + ", ".join(f"{n}={rel_by_slice(lo[n], hi[n], WHOLE):.2g}" for n in LN_TOL) + ")")
