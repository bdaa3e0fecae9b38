"""GPU: every path of flr_bgemm[_ex] and flr_sum_rows[_ex] in the default build.

Structure is checked exactly: on the small-integer operands of
tests/bgemm_ref.py every correct form, tile, split count and summation order
returns the same integers, so the comparison with the int64 reference is
torch.equal.  That covers the 128 x 128 tile with ragged edges, split-K with 2 to
16 splits (even, uneven, on either tile), the three routines that write the
output (the plain linear() stores, BGemm::store_tile, treduce_kernel ->
BGemm::store) with every epilogue, strided and aliased outputs with a NaN
sentinel around them, the operand views the trainers pass, and the workspace
fallback.  The bf16 mid / lo terms are checked on random fp32 operands against
fp64; the kernel forms and knobs against each other bit for bit; the row sums
against the summation order include/flr.h promises, bit for bit.

Each id names the path the shape reaches; bgemm_ref.plan / grid restate the
launch policy and are asserted per case, so a change of the tile or split rule
fails here instead of silently moving a case onto another path."""
import functools

import pytest
import torch
import torch.nn.functional as F

import bgemm_ref as br
from flr import _capi
from flr.nn import bgemm, bgemm_ex, sum_rows

pytestmark = pytest.mark.gpu

NAN = float("nan")
VARIANTS = ("nn", "tn", "nt", "tt", "gather")


# ---- shapes ---------------------------------------------------------------------
# (K, M, N, R, forced tile or None, tile reached, S, store routine of a plain product)
CASES = [
    (2, 130, 200, 260, None, 22, 1, "linear"),    # ragged rows and columns, empty sub-tiles, partial K-tile
    (1, 129, 257, 36, None, 11, 1, "linear"),     # M N < 128 x 512 and R < 256: stays on 64 x 64 tiles
    (1, 129, 257, 36, 22, 22, 1, "linear"),       # ... one row and one column past the 128 tile when forced
    (1, 129, 513, 36, None, 22, 1, "linear"),     # 128 x 128 by the M N rule (R < 256), one row / column past
    (3, 70, 96, 130, None, 11, 1, "linear"),
    (3, 70, 96, 130, 22, 22, 1, "linear"),        # a single partial 128 tile
    (2, 64, 64, 2016, None, 11, 1, "linear"),     # 63 K-tiles: the last shape below the S = 2 threshold
    (2, 64, 64, 2047, None, 11, 2, "treduce"),    # partial last K-tile, R % 4 != 0 (gather mode)
    (2, 60, 68, 2080, None, 11, 2, "treduce"),    # 65 K-tiles (32 + 33), ragged M and N
    (1, 64, 64, 4100, None, 11, 4, "treduce"),    # 129 K-tiles
    (1, 33, 64, 8192, None, 11, 8, "treduce"),
    (1, 64, 40, 16400, None, 11, 16, "treduce"),  # 513 K-tiles
    (2, 130, 200, 2080, None, 22, 2, "treduce"),
    (1, 128, 128, 8192, None, 22, 8, "treduce"),
]


def _id(c):
    K, M, N, R, forced, t, S, store = c
    return f"{K}x{M}x{N}x{R}-{'forced' if forced else ''}tile{t}-S{S}-{store}"


SHALLOW = [c for c in CASES if c[3] <= 2080]
DEEP = [c for c in CASES if c[3] >= 4100]
# grids of 1, 3, 7 and 9 workgroups (64 x 64 tiles, S = 1) for the XCD remap; 3x70x96x130 above has 12
GRIDS = [(1, 40, 50, 100, 1), (3, 33, 40, 100, 3), (7, 20, 30, 50, 7), (1, 130, 190, 100, 9)]
# the shapes of the epilogue tests: one per store routine and tile
EPI_SHAPES = [(3, 70, 96, 130, 11, 1), (2, 130, 200, 260, 22, 1), (2, 60, 68, 2080, 11, 2), (1, 64, 64, 4100, 11, 4)]


def _epi_id(s):
    K, M, N, R, t, S = s
    return f"{K}x{M}x{N}x{R}-tile{t}-S{S}-{'store_tile' if S == 1 else 'treduce'}"


def _reaches(knob, case):
    """Force the case's tile, and assert the path its id names."""
    K, M, N, R, forced, t, S, store = case
    if forced:
        knob("FLR_BGEMM_TILE", str(forced))
    assert br.plan(M, N, R, forced) == (t, S), _id(case)
    assert (store == "treduce") == (S > 1)


# ---- operands -------------------------------------------------------------------
def _kmajor(X):
    """The same values, r-major in memory: the view of a transposed operand."""
    return X.transpose(1, 2).contiguous().transpose(1, 2)


def _spread(X):
    """The same values at every other element of a NaN-filled buffer (gather mode)."""
    buf = torch.full((X.shape[0], X.shape[1], 2 * X.shape[2]), NAN, device=X.device)
    buf[:, :, ::2] = X
    return buf[:, :, ::2]


def _variant(A, B, v):
    if v == "gather":
        A, B = _spread(A), _spread(B)
        assert br.operand_mode(A) == br.operand_mode(B) == "G"
        return A, B
    return (_kmajor(A) if v[0] == "t" else A), (_kmajor(B) if v[1] == "t" else B)


@functools.lru_cache(maxsize=None)
def _rand(K, M, N, R):
    """Random fp32 operands and their fp64 product (computed once per shape)."""
    g = torch.Generator().manual_seed(K * 1000 + M + N + R)
    A, B = torch.randn(K, M, R, generator=g), torch.randn(K, N, R, generator=g)
    return A, B, torch.bmm(A.double(), B.double().transpose(1, 2))


def _err(got, ref):
    return (got.double().cpu() - ref).abs().max().item()


def _scale(ref):
    return max(ref.abs().max().item(), 1.0)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _mm(A, B, **kw):
    """bgemm into an output pre-filled with NaN: an element that is never written
    cannot pass on what an earlier call left in the allocator's memory."""
    out = torch.full((A.shape[0], A.shape[1], B.shape[1]), NAN, device=A.device)
    return bgemm(A, B, out=out, **kw)


def _mmx(A, B, **kw):
    out = torch.full((A.shape[0], A.shape[1], B.shape[1]), NAN, device=A.device)
    return bgemm_ex(A, B, out=out, **kw)


# ---- a. structure, exact -----------------------------------------------------------
@pytest.mark.parametrize("form", ["default", "pipe", "f32"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_structure_exact(cuda, knob, case, form):
    """Integer operands: the product is the int64 reference exactly, in all four
    transposes and through the gather loads, in the default (split at stash), the
    pipelined and the exact-f32 form."""
    K, M, N, R = case[:4]
    _reaches(knob, case)
    if form != "default":
        knob("FLR_GEMM", form)
    o = br.int_operands(K, M, N, R)
    A, B, ref = o["A"].to(cuda), o["B"].to(cuda), o["ref"]
    for v in VARIANTS:
        Av, Bv = _variant(A, B, v)
        C = _mm(Av, Bv).cpu()
        assert torch.equal(C.long(), ref) and torch.equal(C, ref.float()), (v, (C.long() - ref).abs().max().item())


# ---- b. forms and knobs, bit for bit -------------------------------------------------
@pytest.mark.parametrize("case", SHALLOW, ids=_id)
def test_forms_bit_identical(cuda, knob, case):
    """FLR_GEMM unset, stash and pipe give the same bits on random fp32 operands (the
    pipelined form loads through load_op, the default through load_op8)."""
    K, M, N, R = case[:4]
    _reaches(knob, case)
    A, B, _ = _rand(K, M, N, R)
    A, B = A.to(cuda), B.to(cuda)
    for v in VARIANTS:
        Av, Bv = _variant(A, B, v)
        knob("FLR_GEMM", None)
        C0 = _mm(Av, Bv)
        knob("FLR_GEMM", "stash")
        C1 = _mm(Av, Bv)
        knob("FLR_GEMM", "pipe")
        C2 = _mm(Av, Bv)
        assert torch.equal(C0, C1), v
        assert torch.equal(C0, C2), (v, (C0 - C2).abs().max().item())


XCD = [c[:5] + (br.grid(*c[:5]),) for c in SHALLOW] + [g[:4] + (None, g[4]) for g in GRIDS]


@pytest.mark.parametrize("K,M,N,R,forced,wgs", XCD,
                         ids=[f"{K}x{M}x{N}x{R}{'-forcedtile22' if f else ''}-grid{w}" for K, M, N, R, f, w in XCD])
def test_xcd_remap_bit_identical(cuda, knob, K, M, N, R, forced, wgs):
    """FLR_XCD=0 (tiles in grid order) against the default remap, which must be a
    bijection of the grid at any workgroup count (last id field: the grid)."""
    if forced:
        knob("FLR_BGEMM_TILE", str(forced))
    assert br.grid(K, M, N, R, forced) == wgs
    A, B, _ = _rand(K, M, N, R)
    A, B = A.to(cuda), B.to(cuda)
    bias = torch.randn(K, N, device=cuda)
    knob("FLR_XCD", None)
    C1, D1 = _mm(A, B), _mmx(A, B, bias=bias, act="relu")
    knob("FLR_XCD", "0")
    C0, D0 = _mm(A, B), _mmx(A, B, bias=bias, act="relu")
    assert torch.equal(C0, C1) and torch.equal(D0, D1)
    assert not torch.isnan(C1).any()


UNSPLIT = [c for c in SHALLOW if c[4] is None and br.splits(c[1], c[2], c[3], 1) == br.splits(c[1], c[2], c[3], 4) == 1]


@pytest.mark.parametrize("case", UNSPLIT, ids=_id)
def test_tiles_bit_identical(cuda, knob, case):
    """FLR_BGEMM_TILE=11 against 22 wherever neither splits: each accumulator adds
    the same products in the same order on either tile."""
    K, M, N, R = case[:4]
    A, B, _ = _rand(K, M, N, R)
    A, B = A.to(cuda), B.to(cuda)
    for v in VARIANTS:
        Av, Bv = _variant(A, B, v)
        knob("FLR_BGEMM_TILE", "11")
        C11 = _mm(Av, Bv)
        knob("FLR_BGEMM_TILE", "22")
        C22 = _mm(Av, Bv)
        assert torch.equal(C11, C22), (v, (C11 - C22).abs().max().item())


@pytest.mark.parametrize("case", SHALLOW, ids=_id)
def test_f32_form_vs_fp64(cuda, knob, case):
    """FLR_GEMM=f32 (the exact-fp32 MFMA) on random operands, at the bar of the default form."""
    K, M, N, R = case[:4]
    _reaches(knob, case)
    knob("FLR_GEMM", "f32")
    A, B, ref = _rand(K, M, N, R)
    A, B = A.to(cuda), B.to(cuda)
    for v in VARIANTS:
        err = _err(_mm(*_variant(A, B, v)), ref)
        assert err <= 2e-6 * _scale(ref), (v, err, _scale(ref))


# ---- c. epilogues on all three store routines ----------------------------------------
def _place(K, M, N, layout, dev, values=None):
    """(buffer, view): a [K, M, N] view of a NaN-filled buffer.  contig: strides (M N,
    N, 1); transposed: c_m = 1, c_n = M; colslice: columns 5 .. 5 + N of rows N + 11
    wide (c_m > N)."""
    if layout == "colslice":
        buf = torch.full((K, M, N + 11), NAN, device=dev)
        view = buf[:, :, 5:5 + N]
    else:
        buf = torch.full((K * M * N + 64,), NAN, device=dev)
        flat = buf[32:32 + K * M * N]
        view = flat.view(K, M, N) if layout == "contig" else flat.view(K, N, M).transpose(1, 2)
    assert view.shape == (K, M, N)
    if values is not None:
        view.copy_(values)
    return buf, view


def _untouched(buf, view):
    """Every element of buf outside view still holds the NaN sentinel."""
    inside = torch.zeros_like(buf, dtype=torch.bool)
    inside.as_strided(view.size(), view.stride(), view.storage_offset()).fill_(True)
    assert int(inside.sum()) == view.numel()
    return bool(torch.isnan(buf[~inside]).all())


def _run_ex(dev, A, B, o, layout, bias=False, add=False, act="none", mask=False, pre=False, alias=False,
            aux=None):
    """flr_bgemm_ex with every C-shaped argument in `layout` inside its own
    sentinel buffer; returns (out, pre) on the CPU after checking the sentinels and
    that no input was written."""
    K, M, N = A.shape[0], A.shape[1], B.shape[1]
    cbuf, C = _place(K, M, N, layout, dev)
    kw, inputs = {}, []
    if bias:
        kw["bias"] = o["bias"].to(dev)
    if add and alias:
        C.copy_(o["add"])
        kw["add"] = C
    elif add:
        kw["add"] = _place(K, M, N, layout, dev, o["add"])[1]
        inputs.append((kw["add"], o["add"]))
    if mask:
        kw["mul"] = _place(K, M, N, layout, dev, o["mask"])[1]
        inputs.append((kw["mul"], o["mask"]))
    if act in ("drelu", "dgelu", "dtanh"):
        kw["aux"] = _place(K, M, N, layout, dev, o["aux"] if aux is None else aux)[1]
        inputs.append((kw["aux"], o["aux"] if aux is None else aux))
    pbuf = None
    if pre:
        pbuf, kw["pre"] = _place(K, M, N, layout, dev)
    y = bgemm_ex(A, B, act=act, out=C, **kw)
    assert y is C
    assert _untouched(cbuf, C), "a store outside the output view"
    if pre:
        assert _untouched(pbuf, kw["pre"]), "a store outside the pre view"
    for t, want in inputs:
        assert torch.equal(t.cpu(), want), "an epilogue input was written"
    return C.cpu(), (kw["pre"].cpu() if pre else None)


FULL = dict(bias=True, add=True, act="relu", mask=True, pre=True)
INT_EPILOGUES = {
    "none": {},
    "bias": dict(bias=True),                       # off a unit c_n this leaves the linear() stores
    "add": dict(add=True),
    "bias+add": dict(bias=True, add=True),
    "relu": dict(act="relu"),
    "relu*mask": dict(act="relu", mask=True),
    "drelu": dict(act="drelu"),
    "drelu*mask": dict(act="drelu", mask=True),
    "pre": dict(bias=True, pre=True),
    "full": FULL,
    "add=out,relu*mask": dict(bias=True, add=True, alias=True, act="relu", mask=True),  # the trainers' h1 call
    "add=out": dict(add=True, alias=True),
}


@pytest.mark.parametrize("layout", ["contig", "transposed", "colslice"])
@pytest.mark.parametrize("shape", EPI_SHAPES, ids=_epi_id)
def test_epilogues_exact(cuda, knob, shape, layout):
    """Every epilogue on integer operands, exact, in three output layouts, with the
    surroundings of every written view checked.  S = 1 reaches the linear() stores
    (none / bias, unit c_n) and store_tile (the rest); S > 1 treduce -> store."""
    K, M, N, R, t, S = shape
    assert br.plan(M, N, R) == (t, S)
    o = br.int_operands(K, M, N, R)
    A, B = o["A"].to(cuda), o["B"].to(cuda)
    for name, e in INT_EPILOGUES.items():
        got, pre = _run_ex(cuda, A, B, o, layout, **e)
        ref_kw = {k: e[k] for k in ("bias", "add", "act", "mask") if k in e}
        want_pre, want = br.int_epilogue(o, **ref_kw)
        assert torch.equal(got.long(), want) and torch.equal(got, want.float()), \
            (name, (got.long() - want).abs().max().item())
        if e.get("pre"):
            assert torch.equal(pre.long(), want_pre), name


def _gelu_grad64(x):
    x = x.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(F.gelu(x).sum(), x)
    return g


def _fp32_bmm_bar(A, B, ref):
    """The bar for a deep reduction: four times the error of a CPU fp32 torch.bmm on
    the same operands against fp64 (a quantity of the references alone), and never
    less than the shallow shapes' 2e-6 max(|ref|, 1)."""
    yard = (torch.bmm(A, B.transpose(1, 2)).double() - ref).abs().max().item()
    return max(4.0 * yard, 2e-6 * _scale(ref)), yard


@pytest.mark.parametrize("shape", EPI_SHAPES, ids=_epi_id)
def test_epilogue_activations_vs_fp64(cuda, shape):
    """GELU, tanh and their derivative modes on random operands (W scaled by
    1 / sqrt(R): pre-activations of O(1)) with bias, addend and pre.  The bar is the
    product's (2e-6 max(|ref|, 1); at R = 4100 the deep-reduction bar of
    test_numerics_deep); GELU's slope is at most 1.13 and tanh's at most 1, and the
    fp32 erf / tanh / exp add a few 1e-7."""
    K, M, N, R, t, S = shape
    g = torch.Generator().manual_seed(R + M)
    A, W = torch.randn(K, M, R, generator=g), torch.randn(K, N, R, generator=g) / R ** 0.5
    o = {"bias": torch.randn(K, N, generator=g), "add": torch.randn(K, M, N, generator=g)}
    prod = torch.bmm(A.double(), W.double().transpose(1, 2))
    pref = (prod + o["bias"].double().unsqueeze(1)) + o["add"].double()
    bar = _fp32_bmm_bar(A, W, prod)[0] if R >= 4100 else 2e-6 * _scale(prod)
    bar_pre = bar + 2 * 2.0 ** -24 * _scale(pref)  # the bias and the addend: two more fp32 roundings
    Ad, Wd = A.to(cuda), W.to(cuda)
    for act, fn in (("gelu", F.gelu), ("tanh", torch.tanh)):
        y, pre = _run_ex(cuda, Ad, Wd, o, "contig", bias=True, add=True, act=act, pre=True)
        assert _err(pre, pref) <= bar_pre, (act, _err(pre, pref), bar_pre)
        assert _err(y, fn(pref)) <= 1.13 * bar_pre + 1e-6, (act, _err(y, fn(pref)), bar_pre)
    # backward modes: v = (A W^T) * act'(aux); aux = the GELU input / the tanh output
    for act, aux, factor in (("dgelu", pref.float(), _gelu_grad64(pref.float().double())),
                             ("dtanh", torch.tanh(pref).float(), 1.0 - torch.tanh(pref).float().double() ** 2)):
        y, _ = _run_ex(cuda, Ad, Wd, {}, "contig", act=act, aux=aux)
        want = prod * factor
        assert _err(y, want) <= 1.13 * bar + 1e-6 * _scale(prod), (act, _err(y, want))


# ---- d. numerics on random fp32 (the mid / lo terms) -----------------------------------
@pytest.mark.parametrize("case", SHALLOW, ids=_id)
def test_numerics_vs_fp64(cuda, knob, case):
    """The three-term product against fp64 at the project's bar, 2e-6 max(|ref|, 1)."""
    K, M, N, R = case[:4]
    _reaches(knob, case)
    A, B, ref = _rand(K, M, N, R)
    A, B = A.to(cuda), B.to(cuda)
    for v in VARIANTS:
        err = _err(_mm(*_variant(A, B, v)), ref)
        assert err <= 2e-6 * _scale(ref), (v, err, _scale(ref))


@pytest.mark.parametrize("case", DEEP, ids=_id)
def test_numerics_deep(cuda, knob, case):
    """R >= 4100 under split-K.  The bar is four times the error of a CPU fp32
    torch.bmm against fp64 on the same operands (both are fp32 chains of O(sqrt R)
    error, in different orders), and at least 2e-6 max(|ref|, 1).  Printed with -s:
    the kernel's error, the yardstick and the margin.  Measured on MI355X (absolute
    errors; the same in all five operand layouts):

        shape                 S   kernel    fp32 bmm  |ref|max  bar       margin
        1 x 64 x 64 x 4100    4   2.33e-4   7.14e-5   265.0     5.30e-4   2.3x   (the 2e-6 floor)
        1 x 33 x 64 x 8192    8   2.12e-4   9.64e-5   288.2     5.77e-4   2.7x   (the 2e-6 floor)
        1 x 64 x 40 x 16400   16  2.19e-4   7.21e-4   481.5     2.88e-3   13.2x  (4 x fp32 bmm)
        1 x 128 x 128 x 8192  8   2.56e-4   1.18e-4   365.5     7.31e-4   2.9x   (the 2e-6 floor)

    That is 5e-7 to 9e-7 of |ref|max: the deep split reductions stay inside the
    bar the shallow shapes are held to."""
    K, M, N, R = case[:4]
    _reaches(knob, case)
    A, B, ref = _rand(K, M, N, R)
    bar, yard = _fp32_bmm_bar(A, B, ref)
    Ad, Bd = A.to(cuda), B.to(cuda)
    for v in VARIANTS:
        err = _err(_mm(*_variant(Ad, Bd, v)), ref)
        print(f"\n[bgemm {_id(case)} {v}] err {err:.3e}, fp32 bmm {yard:.3e}, bar {bar:.3e}, "
              f"margin {bar / max(err, 1e-30):.1f}x, |ref| {_scale(ref):.1f}")
        assert err <= bar, (v, err, bar)


# ---- e. operand views ----------------------------------------------------------------
@pytest.mark.parametrize("K,M,N,R,t", [(3, 70, 96, 132, 11), (2, 130, 200, 260, 22)],
                         ids=["3x70x96x132-tile11-S1", "2x130x200x260-tile22-S1"])
def test_operand_views_exact(cuda, K, M, N, R, t):
    """The views the trainers pass: a weight slice with an offset base (16-byte
    aligned: still RK; 12 bytes: gather), an operand 4 bytes off, a shared operand
    (b_k = 0) and a shared bias (bias_k = 0).  Everything around the operands is NaN."""
    assert br.plan(M, N, R) == (t, 1)
    o = br.int_operands(K, M, N, R)
    A, B, ref = o["A"].to(cuda), o["B"].to(cuda), o["ref"]
    assert br.operand_mode(A) == br.operand_mode(B) == "RK"

    def inside(X, off, pad):
        buf = torch.full((X.shape[0], X.shape[1], off + X.shape[2] + pad), NAN, device=cuda)
        buf[:, :, off:off + X.shape[2]] = X
        return buf[:, :, off:off + X.shape[2]]
    for name, Av, Bv, modes in (("W[:, :, 64:]", A, inside(B, 64, 0), ("RK", "RK")),
                                ("W[:, :, 3:]", A, inside(B, 3, 0), ("RK", "G")),
                                ("A[:, :, 1:R+1]", inside(A, 1, 3), B, ("G", "RK")),
                                ("both offset", inside(A, 64, 4), inside(B, 8, 0), ("RK", "RK"))):
        assert (br.operand_mode(Av), br.operand_mode(Bv)) == modes, name
        assert torch.equal(_mm(Av, Bv).cpu().long(), ref), name
    # one operand shared by the clients, as either argument; a shared bias
    bias1 = o["bias"][:1].to(cuda)
    Bs, As = B[:1].expand(K, N, R), A[:1].expand(K, M, R)
    assert Bs.stride(0) == 0 and As.stride(0) == 0 and bias1.expand(K, N).stride(0) == 0
    Ai, Bi, bi = o["A"].long(), o["B"].long(), o["bias"][:1].long().unsqueeze(1)
    got = _mm(A, Bs, bias=bias1.expand(K, N)).cpu().long()
    assert torch.equal(got, torch.bmm(Ai, Bi[:1].expand(K, N, R).transpose(1, 2)) + bi)
    got = _mmx(As, B, bias=bias1.expand(K, N), act="relu").cpu().long()
    assert torch.equal(got, (torch.bmm(Ai[:1].expand(K, M, R), Bi.transpose(1, 2)) + bi).clamp(min=0))


# ---- f. batch invariance under split-K ---------------------------------------------------
@pytest.mark.parametrize("M,N,R,t,S", [(130, 200, 2080, 22, 2), (64, 64, 4100, 11, 4)],
                         ids=["130x200x2080-tile22-S2", "64x64x4100-tile11-S4"])
def test_batch_invariant_split_k(cuda, M, N, R, t, S):
    """A client's result (with bias and ReLU, through treduce) has the same bits in a
    launch of 5 clients, of 2, and at another position in the batch."""
    assert br.plan(M, N, R) == (t, S)
    g = torch.Generator().manual_seed(M + R)
    A, B = torch.randn(5, M, R, generator=g).to(cuda), torch.randn(5, N, R, generator=g).to(cuda)
    bias = torch.randn(5, N, generator=g).to(cuda)
    y5 = _mmx(A, B, bias=bias, act="relu")
    assert torch.equal(y5[:2], _mmx(A[:2], B[:2], bias=bias[:2], act="relu"))
    assert torch.equal(y5[3:], _mmx(A[3:], B[3:], bias=bias[3:], act="relu"))
    assert (y5 > 0).any() and (y5 == 0).any()


# ---- g. workspace fallback ---------------------------------------------------------------
def test_workspace_fallback_exact(cuda):
    """Without a workspace, or with one a byte short, flr_bgemm runs unsplit: FLR_OK,
    the exact result, and a short workspace is not written."""
    K, M, N, R = 1, 64, 64, 4100
    assert br.plan(M, N, R) == (11, 4)
    need = int(_capi.lib().flr_bgemm_workspace(K, M, N, R))
    assert need == br.workspace_bytes(K, M, N, R) == 4 * 64 * 64 * 4
    o = br.int_operands(K, M, N, R)
    A, B = o["A"].to(cuda), o["B"].to(cuda)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=cuda)
    for ptr, nbytes in ((None, 0), (None, need), (ws.data_ptr(), need - 1), (ws.data_ptr(), 0)):
        C = torch.full((K, M, N), NAN, device=cuda)
        rc = _capi.call("flr_bgemm", A.data_ptr(), *A.stride(), B.data_ptr(), *B.stride(), C.data_ptr(), *C.stride(),
                        None, 0, None, K, M, N, R, ptr, nbytes, _stream(cuda))
        assert rc == _capi.FLR_OK
        assert torch.equal(C.cpu().long(), o["ref"]), (ptr is None, nbytes)
    assert bool((ws == 0xA5).all())
    # and with the whole workspace: the split path, the same integers
    C = torch.full((K, M, N), NAN, device=cuda)
    _capi.call("flr_bgemm", A.data_ptr(), *A.stride(), B.data_ptr(), *B.stride(), C.data_ptr(), *C.stride(),
               None, 0, None, K, M, N, R, ws.data_ptr(), need, _stream(cuda))
    assert torch.equal(C.cpu().long(), o["ref"])
    assert not bool((ws == 0xA5).all())


# ---- h. non-finite containment -------------------------------------------------------------
@pytest.mark.parametrize("form", ["default", "f32"])
@pytest.mark.parametrize("bad", [NAN, float("inf")], ids=["nan", "inf"])
def test_nonfinite_stays_in_its_row(cuda, knob, bad, form):
    """A NaN in one row of A poisons that output row of its client and nothing else;
    in one row of B, that output column.  Every other element keeps its bits.  For
    +inf only "non-finite" is asserted: the three-term split turns inf into NaN
    (v - bf16(v)), the f32 form keeps inf (or gives NaN against a zero or an
    opposite infinity), and neither is pinned."""
    K, M, N, R = 2, 130, 200, 260
    assert br.plan(M, N, R) == (22, 1)
    if form != "default":
        knob("FLR_GEMM", form)
    A, B, _ = _rand(K, M, N, R)
    A, B = A.to(cuda), B.to(cuda)
    C0 = _mm(A, B)
    assert torch.isfinite(C0).all()

    def hit(C):
        return torch.isnan(C) if bad != bad else ~torch.isfinite(C)
    A1 = A.clone()
    A1[1, 77, 13] = bad
    C1 = _mm(A1, B)
    keep = torch.ones_like(C0, dtype=torch.bool)
    keep[1, 77, :] = False
    assert hit(C1[1, 77, :]).all()
    assert torch.equal(C1[keep], C0[keep])
    B1 = B.clone()
    B1[0, 129, 259] = bad
    C2 = _mm(A, B1)
    keep = torch.ones_like(C0, dtype=torch.bool)
    keep[0, :, 129] = False
    assert hit(C2[0, :, 129]).all()
    assert torch.equal(C2[keep], C0[keep])


# ---- i. row sums, bit-exact ------------------------------------------------------------------
def _sum_rows_direct(dev, X, chunked):
    """flr_sum_rows (chunked=False) / flr_sum_rows_ex with its workspace on X held at
    row stride N + 3, into an output at client stride N + 5; NaN in every pad."""
    K, M, N = X.shape
    xb = torch.full((K, M, N + 3), NAN, device=dev)
    xb[:, :, :N] = X
    ob = torch.full((K + 1, N + 5), NAN, device=dev)
    args = (xb.data_ptr(), xb.stride(0), xb.stride(1), K, M, N, ob.data_ptr(), N + 5)
    if chunked:
        n = int(_capi.lib().flr_sum_rows_workspace(K, M, N))
        assert n == br.sum_rows_workspace_bytes(K, M, N)
        ws = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        _capi.call("flr_sum_rows_ex", *args, ws.data_ptr() if n else None, n, _stream(dev))
    else:
        _capi.call("flr_sum_rows", *args, _stream(dev))
    ob = ob.cpu()
    assert torch.isnan(ob[:K, N:]).all() and torch.isnan(ob[K]).all(), "a store outside the output rows"
    return ob[:K, :N]


SUM_ROWS = [(M, N) for M in (1, 7, 8, 9, 255, 256, 257, 511, 512, 513, 2080) for N in (1, 70, 256, 257)] + \
    [(16384, 70), (16385, 70)]


@pytest.mark.parametrize("M,N", SUM_ROWS, ids=[f"M{m}-N{n}" for m, n in SUM_ROWS])
def test_sum_rows_bit_exact(cuda, M, N):
    """The promised order, bit for bit: eight interleaved accumulators, the M % 8
    tail on accumulators 0.., the fixed tree; with the workspace and 256 < M <=
    16384, per 256-row chunk and the partials in chunk order (M = 16385: 65 chunks,
    so the workspace is given and the one-pass order is expected)."""
    K = 2
    X = torch.randn(K, M, N, generator=torch.Generator().manual_seed(M * 1000 + N))
    one, chunked = br.sum_rows_emulated(X, False), br.sum_rows_emulated(X, True)
    if 256 < M <= 16384 and N > 1:
        assert not torch.equal(one, chunked)  # the two orders can be told apart on this input
    if M > 16384 or M <= 256:
        assert torch.equal(one, chunked)
    Xd = X.to(cuda)
    assert torch.equal(sum_rows(Xd).cpu(), chunked)
    assert torch.equal(_sum_rows_direct(cuda, Xd, False), one)
    assert torch.equal(_sum_rows_direct(cuda, Xd, True), chunked)


@pytest.mark.parametrize("M", [100, 513])
def test_sum_rows_batch_invariant(cuda, M):
    X = torch.randn(5, M, 70, generator=torch.Generator().manual_seed(M)).to(cuda)
    s5 = sum_rows(X)
    assert torch.equal(s5[:1], sum_rows(X[:1]))
    assert torch.equal(s5[4:], sum_rows(X[4:]))
    assert torch.equal(s5.cpu(), br.sum_rows_emulated(X, True))
