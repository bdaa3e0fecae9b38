"""a6 + a7: the fused clip + SGD-momentum step (flr_clip_sgd_step and the
blocked forms, include/flr.h) against the numpy model tests/sgd_ref.py, bit for
bit.  The library builds with -ffp-contract=off and the kernels write every
rounding out, so given the norm a call reports, every parameter, momentum and
exported value is exact; the norm itself (an fp64 sum in the kernel's order) is
held to 1 fp32 ulp of numpy's.  Every float the contract says is not written
holds a NaN sentinel before the call and must hold it afterwards: the whole
x / g / m arenas, the output matrix and norms_out are compared as bit patterns
with what the model says they hold."""
import ctypes

import numpy as np
import pytest
import torch

import sgd_ref
from flr import _capi

pytestmark = pytest.mark.gpu

SENT = np.int32(0x7FC12345)   # a quiet NaN: visible if written over, poisons a result if read and used
POISON = np.float32(np.nan)   # data the step must not read (m on a first step, x_blocks behind a shared source)
SIGN = np.int32(-2 ** 31)
PHASE_NORM, PHASE_UPDATE, PHASE_ALL = 1, 2, 3   # FLR_SGD_PHASE_*

GEOMETRY = [9408, 64, 3, 0, 36864, 1000, 4101, 200000]
# block 0 strided by a multiple of 4 (stays on the 16-B path), the empty block and block 5 by odd amounts
GEOMETRY_STRIDES = [9408 + 16, 64, 3, 5, 36864, 1003, 4101, 200000]
# one float off a 16-B boundary: block 0's g, block 4's m, block 7's x -> those blocks take the scalar path
GEOMETRY_MISALIGN = {("g", 0): 1, ("m", 4): 1, ("x", 7): 1}


def _arr(vals, ct):
    return (ct * len(vals))(*vals)


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _same(name, got, want):
    got, want = got.view(np.int32).ravel(), want.view(np.int32).ravel()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{name}: {bad.size} of {got.size} words differ, first at {bad[0]}: "
                           f"got {got[bad[0]]:#x}, want {want[bad[0]]:#x}")


def ragged_sizes(n, seed, hi=40):
    """n small block sizes, empty ones and multiples of 4 among them."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, hi, n)
    s[::7] = 4 * (s[::7] // 4)
    return [int(v) for v in s]


def scattered_offsets(sizes, seed, start=0):
    """Block j's offset in an output (or shared source) row: shuffled order,
    gaps between the blocks, offsets that are a multiple of 4 and others that
    are not.  Returns (offsets, the row length used)."""
    rng = np.random.default_rng(seed)
    offs, cur = [0] * len(sizes), start
    for i, j in enumerate(rng.permutation(len(sizes))):
        cur = (cur + 3) & ~3
        if i % 3 == 1:
            cur += 1 + i % 2
        offs[int(j)] = cur
        cur += sizes[int(j)] + int(rng.integers(1, 7))
    return offs, cur


class Case:
    """One call's inputs in host arenas (SENT everywhere but the live elements),
    their device copies, the call, and the comparison with the model."""

    def __init__(self, cuda, sizes, K, flags, *, wd=0.0, max_norm=1.0, strides=None, misalign=None, out=None,
                 src=None, normed=None, n_extra=0, gscale=3.0, seed=0, lr=0.05, mom=0.9):
        self.dev, self.sizes, self.K, self.flags = cuda, list(sizes), K, flags
        self.lr, self.mom, self.wd, self.max_norm = lr, mom, wd, max_norm
        self.strides = list(strides) if strides is not None else None
        self.cs = self.strides if strides is not None else self.sizes
        self.out, self.src, self.normed, self.n_extra = out, src, normed, n_extra
        self.first, self.last = bool(flags & 1), bool(flags & 2)
        rng = np.random.default_rng(seed)
        nb, mis = len(sizes), misalign or {}
        # arenas: block j of array a at float offset base[a][j], K client rows and one more of sentinel
        self.base, self.host = {}, {}
        for a in "xgm":
            cur, b = 0, []
            for j in range(nb):
                b.append(cur + mis.get((a, j), 0))
                cur = (b[-1] + (K + 1) * self.cs[j] + 4 + 3) & ~3
            self.base[a] = b
            self.host[a] = np.full(cur + 4, SENT, np.int32)
        shared = [self.first and src is not None and src["offsets"][j] >= 0 for j in range(nb)]
        for j, n in enumerate(sizes):
            x = rng.standard_normal((K, n)).astype(np.float32)
            g = (rng.standard_normal((K, n)) * gscale).astype(np.float32)
            m = rng.standard_normal((K, n)).astype(np.float32)
            self._put(self.host["x"], "x", j, np.full((K, n), POISON) if shared[j] else x)
            self._put(self.host["g"], "g", j, g)
            self._put(self.host["m"], "m", j, np.full((K, n), POISON) if self.first else m)
        self.host["norms"] = np.full(K + 1, SENT, np.int32)
        if out is not None:
            self.host["out"] = np.full((K + 2) * out["ld"] + 8, SENT, np.int32)
        if src is not None:  # ignored on a non-first step: poison, to show it
            v = rng.standard_normal(src["len"]).astype(np.float32) if self.first else np.full(src["len"], POISON)
            self.host["src"] = v.view(np.int32).copy()
        self.gsq = np.zeros(K)          # the whole gradient's sum of squares, fp64
        marked = np.zeros(K)
        for j in range(nb):
            g = self._get(self.host["g"], "g", j).astype(np.float64)
            s = (g * g).sum(axis=1)
            self.gsq += s
            if normed is not None and normed[j]:
                marked += s
        if n_extra > 0:  # the marked blocks' squares as n_extra arbitrary fp64 partials per client
            w = rng.random((K, n_extra)) + 0.01
            self.host["extra"] = (marked[:, None] * (w / w.sum(axis=1, keepdims=True)))

    # block j of an arena as [K, n] floats
    def _get(self, arena, a, j):
        b, cs, n = self.base[a][j], self.cs[j], self.sizes[j]
        return np.stack([arena[b + k * cs: b + k * cs + n] for k in range(self.K)]).view(np.float32)

    def _put(self, arena, a, j, vals):
        b, cs, n = self.base[a][j], self.cs[j], self.sizes[j]
        for k in range(self.K):
            arena[b + k * cs: b + k * cs + n] = np.ascontiguousarray(vals[k], np.float32).view(np.int32)

    def _args(self, j0, j1, upto):
        """The argument list of blocks [j0, j1), up to and including ``upto``."""
        def ptrs(a):
            p0 = self.d[a].data_ptr()
            return _arr([p0 + 4 * b for b in self.base[a][j0:j1]], ctypes.c_void_p)
        args = [ptrs("x"), ptrs("g"), ptrs("m"), _arr(self.sizes[j0:j1], ctypes.c_int64),
                _arr(self.strides[j0:j1], ctypes.c_int64) if self.strides is not None else None,
                j1 - j0, self.K, self.lr, self.mom, self.wd, self.max_norm, self.flags]
        if upto == "blocked":
            return args
        out, src = self.out, self.src
        args += [self.d["out"].data_ptr() if out else None,
                 _arr(out["offsets"][j0:j1], ctypes.c_int64) if out else None,
                 out["ld"] if out else 0, out["nneg"] if out else 0,
                 _arr([int(v) for v in self.normed[j0:j1]], ctypes.c_uint8) if self.normed is not None else None,
                 self.d["extra"].data_ptr() if self.n_extra > 0 else None, self.n_extra]
        if upto == "blocked_x":
            return args
        args += [self.d["src"].data_ptr() if src else None,
                 _arr(src["offsets"][j0:j1], ctypes.c_int64) if src else None]
        return args

    def run(self, entry):
        nb = len(self.sizes)
        self.d = {k: torch.from_numpy(v.copy()).to(self.dev) for k, v in self.host.items()}
        need = int(_capi.lib().flr_clip_sgd_workspace(self.K))
        self.ws = torch.zeros(need if self.max_norm > 0 else 0, dtype=torch.uint8, device=self.dev)
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream
        tail = [self.d["norms"].data_ptr()]
        ws = [self.ws.data_ptr() if self.ws.numel() else None, self.ws.numel(), self.stream]
        if entry == "blocked":
            assert self.out is None and self.src is None and self.normed is None
            _capi.call("flr_clip_sgd_step_blocked", *self._args(0, nb, "blocked"), *tail, *ws)
        elif entry == "blocked_x":
            assert self.src is None
            _capi.call("flr_clip_sgd_step_blocked_x", *self._args(0, nb, "blocked_x"), *tail, *ws)
        elif entry == "blocked_src":
            _capi.call("flr_clip_sgd_step_blocked_src", *self._args(0, nb, "src"), *tail, *ws)
        elif entry == "phase_all":
            _capi.call("flr_clip_sgd_step_phase", *self._args(0, nb, "src"), *tail, PHASE_ALL, *ws)
        else:  # one NORM phase over every block, then UPDATE calls of at most 80 blocks, last chunk first
            assert entry == "phase_split"
            _capi.call("flr_clip_sgd_step_phase", *self._args(0, nb, "src"), *tail, PHASE_NORM, *ws)
            step = sgd_ref.BLOCKS_PER_LAUNCH
            for j0 in reversed(range(0, nb, step)):
                _capi.call("flr_clip_sgd_step_phase", *self._args(j0, min(nb, j0 + step), "src"), None,
                           PHASE_UPDATE, *ws)
        torch.cuda.synchronize(self.dev)
        self.got = {k: v.cpu().numpy() for k, v in self.d.items() if k != "extra"}
        return self

    def check(self, exact_norm=None):
        """exact_norm: the norms a test that knows the sum exactly expects, bit for bit (default: the
        whole gradient's norm from numpy, to 1 ulp)."""
        K, got = self.K, self.got
        # inputs the step only reads
        _same("g", got["g"], self.host["g"])
        if self.src is not None:
            _same("x_src", got["src"], self.host["src"])
        # the norm: 1 ulp of numpy's (the fp64 sums differ by reordering only: < 3e-11 relative for
        # <= 3e5 squares, so the fp32 cast can differ only next to a rounding boundary); then the coefficient
        # from the norm the call reported
        if self.max_norm > 0:
            norms = got["norms"][:K].view(np.float32)
            want = np.sqrt(self.gsq).astype(np.float32) if exact_norm is None else np.float32(exact_norm)
            slack = 1 if exact_norm is None else 0
            assert np.isfinite(norms).all() and (_ulps(norms, want) <= slack).all(), (norms, want)
            assert got["norms"][K] == SENT
            coef = sgd_ref.clip_coef(norms, self.max_norm)
        else:
            _same("norms_out (no clip: not written)", got["norms"], self.host["norms"])
            coef = np.ones(K, np.float32)
        self.coef = coef
        ex, em = self.host["x"].copy(), self.host["m"].copy()
        eo = self.host["out"].copy() if self.out is not None else None
        redirect = self.last and self.out is not None
        for j, n in enumerate(self.sizes):
            if n == 0:
                continue
            x = self._get(self.host["x"], "x", j)
            if self.first and self.src is not None and self.src["offsets"][j] >= 0:
                o = self.src["offsets"][j]
                x = np.broadcast_to(self.host["src"][o:o + n].view(np.float32), (K, n))
            xn, mn = sgd_ref.step(x, self._get(self.host["g"], "g", j), self._get(self.host["m"], "m", j),
                                  coef[:, None], self.lr, self.mom, self.wd, self.first)
            assert np.isfinite(xn).all() and np.isfinite(mn).all()
            if not self.last:
                self._put(em, "m", j, mn)
            if redirect:
                o, ld = self.out["offsets"][j], self.out["ld"]
                for k in range(K):
                    bits = xn[k].view(np.int32)
                    eo[k * ld + o: k * ld + o + n] = bits ^ SIGN if k < self.out["nneg"] else bits
            else:
                self._put(ex, "x", j, xn)
        _same("x", got["x"], ex)
        _same("m", got["m"], em)
        if eo is not None:
            _same("x_out", got["out"], eo)
        return self


def _identical(a, b, keys=("x", "m", "norms")):
    for k in keys:
        _same(f"{k} (two runs)", a.got[k], b.got[k])


# ---- the flat form -------------------------------------------------------
@pytest.mark.parametrize("mode", ["first_wd_clip", "middle_clip", "middle_wd_noclip"])
@pytest.mark.parametrize("P", [1, 255, 4099])
def test_flat_step(cuda, P, mode):
    """flr_clip_sgd_step on a K x P matrix of row stride P + 5."""
    K, ld = 3, P + 5
    first = mode.startswith("first")
    wd = 5e-4 if "wd" in mode else 0.0
    max_norm = 0.0 if "noclip" in mode else 0.5
    lr, mom = 0.05, 0.9
    rng = np.random.default_rng(P)
    host = {a: np.full((K + 1, ld), SENT, np.int32) for a in "xgm"}
    x, m = (rng.standard_normal((K, P)).astype(np.float32) for _ in range(2))
    g = ((np.abs(rng.standard_normal((K, P))) * 3.0 + 1.0) * rng.choice([-1.0, 1.0], (K, P))).astype(np.float32)
    host["x"][:K, :P], host["g"][:K, :P] = x.view(np.int32), g.view(np.int32)
    host["m"][:K, :P] = (np.full((K, P), POISON) if first else m).view(np.int32)
    host["norms"] = np.full(K + 1, SENT, np.int32)
    d = {k: torch.from_numpy(v.copy()).to(cuda) for k, v in host.items()}
    need = int(_capi.lib().flr_clip_sgd_workspace(K))
    ws = torch.zeros(need, dtype=torch.uint8, device=cuda) if max_norm > 0 else None
    _capi.call("flr_clip_sgd_step", d["x"].data_ptr(), d["g"].data_ptr(), d["m"].data_ptr(), K, P, ld, lr, mom, wd,
               max_norm, int(first), d["norms"].data_ptr(), ws.data_ptr() if ws is not None else None,
               need if ws is not None else 0, torch.cuda.current_stream(cuda).cuda_stream)
    torch.cuda.synchronize(cuda)
    got = {k: v.cpu().numpy() for k, v in d.items()}
    _same("g", got["g"], host["g"])
    if max_norm > 0:
        norms = got["norms"][:K].view(np.float32)
        want = np.sqrt((g.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)
        assert (_ulps(norms, want) <= 1).all(), (norms, want)
        assert got["norms"][K] == SENT
        assert (norms > max_norm).all()  # the clip is active
        coef = sgd_ref.clip_coef(norms, max_norm)
    else:
        _same("norms_out", got["norms"], host["norms"])
        coef = np.ones(K, np.float32)
    xn, mn = sgd_ref.step(x, g, m, coef[:, None], lr, mom, wd, first)
    ex, em = host["x"].copy(), host["m"].copy()
    ex[:K, :P], em[:K, :P] = xn.view(np.int32), mn.view(np.int32)
    _same("x", got["x"], ex)
    _same("m", got["m"], em)


# ---- block geometry, alignment, strides, step flags, weight decay --------
@pytest.mark.parametrize("wd", [0.0, 5e-4])
@pytest.mark.parametrize("flags", [0, 1, 2, 3], ids=["middle", "first", "last", "both"])
@pytest.mark.parametrize("layout", ["aligned", "misaligned", "strided"])
def test_block_geometry(cuda, layout, flags, wd):
    """An empty block, sizes not a multiple of 4, a part below one workgroup's
    8192 floats, a block long enough for the 8-deep float4 loop and its
    single-group tail; every base 16-B aligned, three bases one float off, and
    client strides above the size.  First steps start from a NaN momentum
    buffer; last steps must leave the buffer alone."""
    kw = {}
    if layout == "misaligned":
        kw["misalign"] = GEOMETRY_MISALIGN
    if layout == "strided":
        kw["strides"] = GEOMETRY_STRIDES
    c = Case(cuda, GEOMETRY, 3, flags, wd=wd, max_norm=1.0, **kw).run("blocked").check()
    assert (c.coef < 1).all()  # the clip is active


@pytest.mark.parametrize("wd", [0.0, 5e-4])
def test_inactive_clip_is_no_clip(cuda, wd):
    """Every norm below max_norm: the coefficient is exactly 1 and the step is
    the max_norm = 0 step (null workspace, norms_out untouched) bit for bit."""
    a = Case(cuda, GEOMETRY, 3, 0, wd=wd, max_norm=1e4, misalign=GEOMETRY_MISALIGN).run("blocked").check()
    assert (a.coef == 1).all()
    b = Case(cuda, GEOMETRY, 3, 0, wd=wd, max_norm=0.0, misalign=GEOMETRY_MISALIGN).run("blocked").check()
    _identical(a, b, keys=("x", "m"))


# ---- more blocks than one launch's table ---------------------------------
@pytest.mark.parametrize("nb,K,flags", [(83, 3, 0), (165, 3, 1), (165, 5, 0), (sgd_ref.MAX_BLOCKS, 2, 0)],
                         ids=["83", "165_first", "165_K5", "limit"])
def test_many_blocks(cuda, nb, K, flags):
    """2, 3 and the limit's 8 tables of 80 blocks: the one call equals the
    model, and equals bit for bit one NORM phase over every block followed by
    UPDATE calls of at most 80 blocks."""
    sizes = ragged_sizes(nb, seed=nb)
    one = Case(cuda, sizes, K, flags, wd=5e-4, max_norm=1.0, seed=nb).run("phase_all").check()
    assert (one.coef < 1).all()
    two = Case(cuda, sizes, K, flags, wd=5e-4, max_norm=1.0, seed=nb).run("phase_split").check()
    _identical(one, two)


def test_many_blocks_through_the_wrapper(cuda):
    Case(cuda, ragged_sizes(165, 1), 3, 0, max_norm=1.0, seed=4).run("blocked").check()


# ---- the redirected last step ---------------------------------------------
@pytest.mark.parametrize("ld_odd", [False, True], ids=["ld4", "ldodd"])
@pytest.mark.parametrize("nneg", [0, 1, 3, 5])  # 0, 1, K, K + 2
@pytest.mark.parametrize("flags", [2, 3], ids=["last", "both"])
def test_redirected_last_step(cuda, flags, nneg, ld_odd):
    """The last step writes the client-matrix rows instead of x_blocks: blocks
    at shuffled offsets with gaps, 16-B aligned and not, rows k < nneg with the
    sign bit flipped; x_blocks, m and the gaps keep what they held."""
    K = 3
    offs, end = scattered_offsets(GEOMETRY, seed=11, start=4)
    ld = ((end + 3) & ~3) + (1 if ld_odd else 0)
    assert sum(o % 4 == 0 for o in offs) >= 2 and sum(o % 4 != 0 for o in offs) >= 2
    out = dict(offsets=offs, ld=ld, nneg=nneg)
    Case(cuda, GEOMETRY, K, flags, wd=5e-4, max_norm=1.0, out=out).run("blocked_x").check()


def test_negated_rows_flip_the_sign_of_zeros(cuda):
    """Zero gradients on +0.0 / -0.0 parameters: the step keeps each zero, the
    rows below nneg export it with the sign bit flipped."""
    K, n = 3, 8
    z = Case(cuda, [n, 5], K, 3, max_norm=0.0, out=dict(offsets=[8, 1], ld=20, nneg=2))
    zero = np.zeros((K, n), np.float32)
    zero[:, ::2] = -0.0
    z._put(z.host["x"], "x", 0, zero)
    z._put(z.host["g"], "g", 0, np.zeros((K, n), np.float32))
    z.run("blocked_x").check()
    rows = z.got["out"][: K * 20].reshape(K, 20)[:, 8:8 + n]
    kept = zero.view(np.int32)
    assert (rows[2] == kept[2]).all() and (rows[0] == kept[0] ^ SIGN).all() and (rows[1] == kept[1] ^ SIGN).all()
    assert set(rows[0].tolist()) == {0, int(SIGN)}


@pytest.mark.parametrize("flags", [0, 1], ids=["middle", "first"])
def test_output_matrix_untouched_before_the_last_step(cuda, flags):
    offs, end = scattered_offsets(GEOMETRY, seed=11)
    out = dict(offsets=offs, ld=(end + 3) & ~3, nneg=1)
    Case(cuda, GEOMETRY, 3, flags, max_norm=1.0, out=out).run("blocked_x").check()


# ---- the shared first-step source -----------------------------------------
@pytest.mark.parametrize("flags", [1, 3, 0, 2], ids=["first", "both_redirected", "middle_ignored", "last_ignored"])
def test_shared_first_step_source(cuda, flags):
    """First step: blocks with src_offsets[j] >= 0 read x_src (their x_blocks
    hold NaN), the ones at -1 read x_blocks, in one call; on a step that is
    also the last, the output offsets are the source's.  Later steps ignore
    x_src (it holds NaN then)."""
    K = 3
    offs, end = scattered_offsets(GEOMETRY, seed=5)
    ld = (end + 3) & ~3
    soffs = [o if j % 3 != 1 else -1 for j, o in enumerate(offs)]
    assert any(o >= 0 and o % 4 for o in soffs) and any(o >= 0 and o % 4 == 0 for o in soffs)
    src = dict(offsets=soffs, len=ld)
    out = dict(offsets=offs, ld=ld, nneg=1) if flags & 2 else None
    Case(cuda, GEOMETRY, K, flags, wd=5e-4, max_norm=1.0, src=src, out=out,
         misalign={("g", 1): 1}).run("blocked_src").check()


# ---- clip norms from producer partials --------------------------------------
@pytest.mark.parametrize("n_extra", [1, 5, 300])
@pytest.mark.parametrize("nb", [10, 165])
def test_producer_partials(cuda, nb, n_extra):
    """A third of the blocks leave their squares to extra_sq (n_extra fp64
    partials per client; 300 wraps the 256-thread sum); the rest are re-packed
    into their own tables for the optimizer's sum (165 blocks: across tables).
    The norm is the whole gradient's; the update is exact from it."""
    sizes = GEOMETRY + [777, 12] if nb == 10 else ragged_sizes(nb, seed=3, hi=200)
    normed = [j % 3 == 1 for j in range(nb)]
    c = Case(cuda, sizes, 3, 0, wd=5e-4, max_norm=1.0, normed=normed, n_extra=n_extra).run("blocked_x").check()
    assert (c.coef < 1).all()


@pytest.mark.parametrize("n_extra", [0, 7])
def test_every_block_normed(cuda, n_extra):
    """No block left for the optimizer's own pass: the norm is the partials'
    (n_extra = 0: the norm is 0 and the coefficient 1)."""
    sizes = ragged_sizes(12, seed=8, hi=300)
    c = Case(cuda, sizes, 3, 1, max_norm=1.0, normed=[True] * 12, n_extra=n_extra).run("phase_all")
    c.check(exact_norm=np.zeros(3) if n_extra == 0 else None)
    if n_extra == 0:
        assert (c.got["norms"][:3] == 0).all() and (c.coef == 1).all()


def test_partial_sum_order(cuda):
    """"Summed per client in a fixed order" (flr.h), the order train_step.hip
    documents: the optimizer's own pass leaves NBLK = 32 sums per client and
    table, number b over the flattened range [P b / 32, P (b + 1) / 32) of the
    blocks without producer partials; one 256-thread workgroup per client then
    takes those followed by the n_extra producer partials, thread t adding
    numbers t, t + 256, ... in turn, and halves the 256 sums (t += t + 128, 64,
    ..., 1).  A sum of squares is too well conditioned for its order to show in
    an fp32 norm, so this test makes it show: integer gradients (each of the 32
    sums is exact in any order), and producer partials +2^(54 + t % 8) that meet
    sum number t in thread t, with their negatives in thread t + 128.  Sum t is
    thereby rounded to a multiple of 2^(2 + t % 8) and the total is an integer
    that depends on which thread took which sum.  The norm is then exact, not
    within 1 ulp; the update follows from it as everywhere else."""
    K, n_extra, nblk, threads = 2, 300, 32, 256
    sizes = [4000, 1001, 500, 13000, 7, 14000]
    normed = [False, False, True, False, False, False]
    c = Case(cuda, sizes, K, 0, wd=5e-4, max_norm=1.0, normed=normed, n_extra=n_extra, seed=21)
    rng = np.random.default_rng(21)
    for j, n in enumerate(sizes):
        c._put(c.host["g"], "g", j, rng.integers(-8, 9, (K, n)).astype(np.float32))
    extra = np.zeros((K, n_extra))
    for t in range(nblk):
        extra[:, t + threads - nblk] = 2.0 ** (54 + t % 8)   # number t + 256: thread t, after sum t
        extra[:, t + 128 - nblk] = -2.0 ** (54 + t % 8)       # number t + 128: thread t + 128, alone
    marked = c._get(c.host["g"], "g", 2).astype(np.float64)
    extra[:, 0] = (marked * marked).sum(axis=1)              # number 32: thread 32
    c.host["extra"] = extra
    c.run("blocked_x")
    want = np.zeros(K, np.float32)
    for k in range(K):
        flat = np.concatenate([c._get(c.host["g"], "g", j)[k] for j in range(len(sizes)) if not normed[j]])
        sq = flat.astype(np.float64) ** 2
        P = sq.size
        nums = [sq[P * b // nblk: P * (b + 1) // nblk].sum() for b in range(nblk)] + list(extra[k])
        red = np.array([sum(nums[t::threads], 0.0) for t in range(threads)])
        o = threads // 2
        while o:
            red[:o] += red[o:2 * o]
            o //= 2
        want[k] = np.float32(np.sqrt(red[0]))
        assert red[0] != sq.sum() + extra[k, 0]  # the rounding happened: the order is visible
    c.check(exact_norm=want)
