"""a3: every GRU step kernel of csrc/train_gru.hip, one step at a time, through
the C entries: the weight packer, the fused recurrence steps in each compiled
form (FLR_GRU_FW / FLR_GRU_BW), shared weights, dh0, and the two pointwise
kernels, against the fp64 restatement in tests/gru_ref.py
(test_gru_ref_host.py pins that to torch.nn.GRU and autograd).

Every buffer of a call is a slice of one allocation ("arena") with at least
1024 floats of a NaN pattern on both sides; outputs and every time slot the
call must not touch are prefilled with another NaN pattern.  After each call
everything outside the slots the call owns holds its bits, and everything
inside them was written.

Bounds.  r, z, n, h', dgh, dgi, dh_direct: the project's 2e-6 * max(scale, 1)
per tensor (test_gpu_gru.py's bar for a whole sweep).  The GEMM results that are
visible on their own (hn forward, dh0 backward) are held elementwise to
  |got - ref| <= c * 2^-24 * (|addend| + sum_r |a_r| |w_r|),
c = 4 x the largest such ratio of a plain fp32 CPU matmul of the same operands
at that shape (floor 4), computed here from the CPU run.  Measured ratios:
profiles/gru_steps/README.md."""
import functools
import math
import types

import pytest
import torch

import gru_ref
from flr import _capi
from flr.nn import _gru_packed, bgemm

pytestmark = pytest.mark.gpu

SHAPES = [  # (K, B, T, H)
    (1, 1, 2, 1),      # everything degenerate; scalar-load path; one lane of one tile live
    (3, 5, 3, 24),     # vector-load path, H % 16 == 8, 2 k-steps for 8 waves; backward R = 72
    (2, 32, 3, 40),    # full batch; second unit block ragged (8 of 32 units)
    (3, 17, 3, 37),    # scalar-load path; B crosses 16; ragged unit block
    (8, 4, 2, 96),     # grid 24: XCD remap on, 3 blocks per client
    (2, 32, 2, 300),   # 19 / 57 k-steps: every form's last load group partial; 16,3's last wave idle
]
FW_FORMS = ["8,2", "4,4", "2,8", "8,2s"]            # "8,2" is the default
BW_FORMS = ["8,2", "8,2s", "8,6", "4,12", "16,3"]
BW_SAME_ORDER = ("8,2s", "8,6")                     # 8 waves: the default's summation order
MARGIN = 1024
MARGIN_BITS = 0x7FCA11CE   # quiet NaNs with payloads: nothing computes these
PREFILL_BITS = 0x7FC5A5A5
FLR_ERR_ARG = -1
U = 2.0 ** -24


def _ids(xs):
    return [str(x).replace(" ", "") for x in xs]


def prefilled(*shape):
    return torch.full(shape, PREFILL_BITS, dtype=torch.int32).view(torch.float32)


def bits(t):
    return t.contiguous().view(torch.int32)


class Arena:
    """One device allocation holding the call's buffers (CPU fp32 tensors, in
    the order given) with margins between and around them."""

    def __init__(self, dev, **bufs):
        self.span, off = {}, MARGIN
        for name, t in bufs.items():
            self.span[name] = (off, tuple(t.shape))
            off += -(-t.numel() // 64) * 64 + MARGIN   # every buffer starts 256-byte aligned
        self.before = torch.full((off,), MARGIN_BITS, dtype=torch.int32)
        for name, t in bufs.items():
            o = self.span[name][0]
            self.before[o:o + t.numel()] = bits(t).reshape(-1)
        self.owned = torch.zeros(off, dtype=torch.bool)
        self.dev = self.before.to(dev)
        self.after = None

    def ptr(self, name):
        return self.dev.data_ptr() + 4 * self.span[name][0]

    def own(self, name, *index):
        """The call may (and must) write buf[index]."""
        o, shape = self.span[name]
        m = torch.zeros(shape, dtype=torch.bool)
        m[index if index else ...] = True
        self.owned[o:o + m.numel()] |= m.reshape(-1)

    def check(self):
        """Fetch the arena; nothing outside the owned slots changed (margins,
        inputs, other time slots) and every owned element was written."""
        self.after = self.dev.cpu()
        changed = (self.after != self.before) & ~self.owned
        if changed.any():
            where = []
            for name, (o, shape) in self.span.items():
                n = math.prod(shape)
                if changed[o:o + n].any():
                    where.append(name)
            first = int(changed.nonzero()[0])
            raise AssertionError(f"{int(changed.sum())} floats outside the call's slots changed, first at arena "
                                 f"offset {first}; in buffers {where or 'none (margins only)'}")
        stale = self.owned & (self.after == PREFILL_BITS)
        assert not stale.any(), f"{int(stale.sum())} owned output floats were never written"

    def get(self, name):
        o, shape = self.span[name]
        n = math.prod(shape)
        return self.after[o:o + n].view(torch.float32).reshape(shape).clone()


def stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def case(shape):
    """The inputs of every test at this shape: seeded CPU normals, drawn once."""
    K, B, T, H = shape
    g = torch.Generator().manual_seed(K * 100003 + B * 1009 + T * 101 + H)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    c = types.SimpleNamespace(K=K, B=B, T=T, H=H)
    c.gi = rn(K, B, T, 3 * H)
    c.whh = rn(K, 3 * H, H) * H ** -0.5
    c.bhh = rn(K, 3 * H)
    c.h = rn(K, T + 1, B, H)                       # slot t is the h_t a call at t reads: non-zero
    c.gates = torch.stack([torch.sigmoid(rn(K, T, B, H)), torch.sigmoid(rn(K, T, B, H)),
                           torch.tanh(rn(K, T, B, H)), rn(K, T, B, H)], 3)   # [K][T][B][4][H]: r, z, n, hn
    c.dgh = rn(K, T, B, 3 * H)
    c.dhd = rn(K, B, H)                            # dh_direct going in
    c.dh = rn(K, B, H)                             # dL/dh_{t+1} of the unfused backward
    c.gh = rn(K, B, 3 * H)                         # the unfused forward's hidden projection
    c.whhP = gru_ref.pack(c.whh, 3, H, H, 0)
    c.whhTP = gru_ref.pack(c.whh, 1, H, 3 * H, 1)
    return c


def clients(c, n):
    """The first n clients of a case, as a case."""
    d = types.SimpleNamespace(K=n, B=c.B, T=c.T, H=c.H)
    for name, v in vars(c).items():
        if torch.is_tensor(v):
            setattr(d, name, v[:n].contiguous())
    return d


def only_slot(x, dim, t):
    """x with every index of `dim` but t replaced by the prefill pattern."""
    out = prefilled(*x.shape)
    idx = [slice(None)] * x.dim()
    idx[dim] = t
    out[tuple(idx)] = x[tuple(idx)]
    return out


# ---- the launches -----------------------------------------------------------

def run_fwd_fused(dev, c, t, whhP=None, shared=None):
    """One fused forward step; returns (r, z, n, hn, h_next) as written.
    shared None: flr_gru_fwd_fused; 0 / 1: flr_gru_fwd_fused_ex."""
    K, B, T, H = c.K, c.B, c.T, c.H
    a = Arena(dev, whhP=c.whhP if whhP is None else whhP, gi=c.gi, bhh=c.bhh, hseq=only_slot(c.h, 1, t),
              gates=prefilled(K, T, B, 4, H))
    a.own("hseq", slice(None), t + 1)
    a.own("gates", slice(None), t)
    if shared is None:
        _capi.call("flr_gru_fwd_fused", a.ptr("gi"), a.ptr("whhP"), a.ptr("bhh"), a.ptr("hseq"), a.ptr("gates"),
                   K, B, T, H, t, stream())
    else:
        _capi.call("flr_gru_fwd_fused_ex", a.ptr("gi"), a.ptr("whhP"), shared, a.ptr("bhh"), a.ptr("hseq"),
                   a.ptr("gates"), K, B, T, H, t, stream())
    a.check()
    gt = a.get("gates")[:, t]
    return gt[:, :, 0], gt[:, :, 1], gt[:, :, 2], gt[:, :, 3], a.get("hseq")[:, t + 1]


def bwd_buffers(c, t):
    """The backward buffers of a call whose element backward is step t
    (reads gates[:, t], hseq[:, t]; the fused call at t + 1 also dgh[:, t + 1])."""
    K, B, T, H = c.K, c.B, c.T, c.H
    return dict(gates=only_slot(c.gates, 1, t), hseq=only_slot(c.h, 1, t),
                dgh=only_slot(c.dgh, 1, t + 1) if t + 1 < T else prefilled(K, T, B, 3 * H),
                dgi=prefilled(K, B, T, 3 * H))


def run_bwd_fused(dev, c, t, with_dh0=True, whhTP=None, shared=None):
    """One fused backward step t >= 1; returns (dh0 | None, dgh[:, t-1],
    dgi[:, :, t-1], dh_direct) as written."""
    K, B, T, H = c.K, c.B, c.T, c.H
    bufs = dict(whhTP=c.whhTP if whhTP is None else whhTP, **bwd_buffers(c, t - 1), dhd=c.dhd)
    if with_dh0:
        bufs["dh0"] = prefilled(K, B, H)
    a = Arena(dev, **bufs)
    a.own("dgh", slice(None), t - 1)
    a.own("dgi", slice(None), slice(None), t - 1)
    a.own("dhd")
    if with_dh0:
        a.own("dh0")
    dh0 = a.ptr("dh0") if with_dh0 else None
    if shared is None:
        _capi.call("flr_gru_bwd_fused", a.ptr("whhTP"), a.ptr("gates"), a.ptr("hseq"), a.ptr("dgh"), a.ptr("dgi"),
                   a.ptr("dhd"), dh0, K, B, T, H, t, stream())
    else:
        _capi.call("flr_gru_bwd_fused_ex", a.ptr("whhTP"), shared, a.ptr("gates"), a.ptr("hseq"), a.ptr("dgh"),
                   a.ptr("dgi"), a.ptr("dhd"), dh0, K, B, T, H, t, stream())
    a.check()
    return (a.get("dh0") if with_dh0 else None, a.get("dgh")[:, t - 1], a.get("dgi")[:, :, t - 1], a.get("dhd"))


def run_fwd_step(dev, c, t, gh):
    K, B, T, H = c.K, c.B, c.T, c.H
    a = Arena(dev, gi=c.gi, gh=gh, hseq=only_slot(c.h, 1, t), gates=prefilled(K, T, B, 4, H))
    a.own("hseq", slice(None), t + 1)
    a.own("gates", slice(None), t)
    _capi.call("flr_gru_fwd_step", a.ptr("gi"), a.ptr("gh"), a.ptr("hseq"), a.ptr("gates"), K, B, T, H, t, stream())
    a.check()
    gt = a.get("gates")[:, t]
    return gt[:, :, 0], gt[:, :, 1], gt[:, :, 2], gt[:, :, 3], a.get("hseq")[:, t + 1]


def run_bwd_step(dev, c, t, dh):
    """The unfused element backward of step t; returns (dgh[:, t], dgi[:, :, t], dh_direct)."""
    K, B, T, H = c.K, c.B, c.T, c.H
    a = Arena(dev, dh=dh, **bwd_buffers(c, t), dhd=prefilled(K, B, H))
    a.own("dgh", slice(None), t)
    a.own("dgi", slice(None), slice(None), t)
    a.own("dhd")
    _capi.call("flr_gru_bwd_step", a.ptr("dh"), a.ptr("gates"), a.ptr("hseq"), a.ptr("dgh"), a.ptr("dgi"),
               a.ptr("dhd"), K, B, T, H, t, stream())
    a.check()
    return a.get("dgh")[:, t], a.get("dgi")[:, :, t], a.get("dhd")


# ---- references and bounds --------------------------------------------------

def fwd_ref_of(c, t, gh=None):
    """fp64 (r, z, n, hn, h_next); gh given: the pointwise part alone on that gh."""
    H = c.H
    if gh is None:
        return gru_ref.fwd_step(c.gi[:, :, t].double(), c.h[:, t].double(), c.whh.double(), c.bhh.double())
    gi, g, h = c.gi[:, :, t].double(), gh.double(), c.h[:, t].double()
    r = torch.sigmoid(gi[..., :H] + g[..., :H])
    z = torch.sigmoid(gi[..., H:2 * H] + g[..., H:2 * H])
    hn = g[..., 2 * H:]
    n = torch.tanh(gi[..., 2 * H:] + r * hn)
    return r, z, n, hn, (h - n) * z + n


@functools.lru_cache(maxsize=None)
def fwd_ref(shape, t):
    c = case(shape)
    H = c.H
    ref = fwd_ref_of(c, t)
    h, wn, bn = c.h[:, t], c.whh[:, 2 * H:], c.bhh[:, None, 2 * H:]
    unit = U * (bn.double().abs() + gru_ref.abs_products(h.double(), wn.double()))
    cpu32 = torch.matmul(h, wn.transpose(1, 2)) + bn          # plain fp32 on the CPU
    ratio = ((cpu32.double() - ref[3]).abs() / unit).max().item()
    return ref, unit, ratio


def bwd_ref_of(c, t, dh_t=None):
    """fp64 (dh_t, dgh[:, t-1], dgi[:, :, t-1], dh_direct) of the fused step t."""
    if dh_t is None:
        dh_t = gru_ref.bwd_gemm(c.dhd.double(), c.dgh[:, t].double(), c.whh.double())
    g = c.gates[:, t - 1].double()
    return (dh_t,) + gru_ref.bwd_step(dh_t, g[:, :, 0], g[:, :, 1], g[:, :, 2], g[:, :, 3], c.h[:, t - 1].double())


@functools.lru_cache(maxsize=None)
def bwd_ref(shape, t):
    c = case(shape)
    ref = bwd_ref_of(c, t)
    a, wt = c.dgh[:, t], c.whh.transpose(1, 2)                # dgh_t [K][B][3H] x (W_hh^T) [K][H][3H]
    unit = U * (c.dhd.double().abs() + gru_ref.abs_products(a.double(), wt.double()))
    cpu32 = c.dhd + torch.matmul(a, c.whh)
    ratio = ((cpu32.double() - ref[0]).abs() / unit).max().item()
    return ref, unit, ratio


def gemm_c(cpu_ratio):
    return max(4.0, 4.0 * cpu_ratio)


def assert_tensor(name, got, want, factor=1.0):
    """The project's per-tensor bound."""
    err = (got.double() - want).abs().max().item()
    scale = want.abs().max().item()
    print(f"  {name}: err {err:.3e} scale {scale:.3e}")
    assert err <= factor * 2e-6 * max(scale, 1.0), (name, err, scale)


def assert_gemm(tag, got, want, unit, cpu_ratio):
    ratio = ((got.double() - want).abs() / unit)
    worst = ratio.max().item()
    print(f"RATIO {tag} cpu {cpu_ratio:.3f} kernel {worst:.3f} c {gemm_c(cpu_ratio):.3f}")
    ok = ratio <= gemm_c(cpu_ratio)     # a NaN compares false
    assert ok.all(), (tag, worst, gemm_c(cpu_ratio), int((~ok).sum()), (~ok).nonzero()[0].tolist())


def assert_same_bits(names, got, want):
    for name, g, w in zip(names, got, want):
        assert torch.equal(bits(g), bits(w)), f"{name}: {int((bits(g) != bits(w)).sum())} of {g.numel()} floats differ"


FWD_NAMES = ("r", "z", "n", "hn", "h_next")
BWD_NAMES = ("dgh", "dgi", "dh_direct")


def fwd_steps(shape):
    return sorted({0, shape[2] - 1})


def bwd_steps(shape):
    return sorted({1, shape[2] - 1})


# ---- 1. the packer ----------------------------------------------------------

PACKS = sorted({(3, s[3], s[3], 0) for s in SHAPES} | {(1, s[3], 3 * s[3], 1) for s in SHAPES}) + [
    (1, 33, 130, 0), (1, 33, 130, 1)]   # C crosses the packer's 128-column chunk; 9 k-steps


@pytest.mark.parametrize("dims", PACKS, ids=_ids(PACKS))
def test_pack_layout_bit_exact(cuda, dims):
    NG, H, C, trans = dims
    K = 3
    g = torch.Generator().manual_seed(NG * 7 + H * 11 + C * 13 + trans)
    w = torch.randn(K, NG * H * C, generator=g)
    a = Arena(cuda, w=w, wp=prefilled(K, _gru_packed(NG, H, C)))
    a.own("wp")
    _capi.call("flr_gru_pack", a.ptr("w"), K, NG, H, C, trans, a.ptr("wp"), stream())
    a.check()
    want = gru_ref.pack(w, NG, H, C, trans)
    got = a.get("wp")
    assert torch.equal(bits(got), bits(want)), f"{int((bits(got) != bits(want)).sum())} packed floats differ"


# ---- 2. the fused forward step ----------------------------------------------

@pytest.mark.parametrize("form", FW_FORMS, ids=_ids(FW_FORMS))
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_fwd_fused_step_vs_fp64(cuda, knob, shape, form):
    c = case(shape)
    for t in fwd_steps(shape):
        knob("FLR_GRU_FW", form)
        got = run_fwd_fused(cuda, c, t)
        ref, unit, cpu_ratio = fwd_ref(shape, t)
        assert_gemm(f"fwd {shape} {form} t={t}", got[3], ref[3], unit, cpu_ratio)
        for name, g, w in zip(FWD_NAMES, got, ref):
            if name != "hn":
                assert_tensor(name, g, w)
        if form == "8,2s":   # the source's claim: the ordered one-slot reduction is the default's sum
            knob("FLR_GRU_FW", "8,2")
            assert_same_bits(FWD_NAMES, got, run_fwd_fused(cuda, c, t))


# ---- 3. the fused backward step ---------------------------------------------

BW_CASES = [s for s in SHAPES if s[2] >= 2]


@pytest.mark.parametrize("form", BW_FORMS, ids=_ids(BW_FORMS))
@pytest.mark.parametrize("shape", BW_CASES, ids=_ids(BW_CASES))
def test_bwd_fused_step_vs_fp64(cuda, knob, shape, form):
    c = case(shape)
    for t in bwd_steps(shape):
        knob("FLR_GRU_BW", form)
        dh0, *got = run_bwd_fused(cuda, c, t)
        ref, unit, cpu_ratio = bwd_ref(shape, t)
        assert_gemm(f"bwd {shape} {form} t={t}", dh0, ref[0], unit, cpu_ratio)
        for name, g, w in zip(BWD_NAMES, got, ref[1:]):
            assert_tensor(name, g, w)
        # dh0 is optional: without it the step is the same
        assert_same_bits(BWD_NAMES, run_bwd_fused(cuda, c, t, with_dh0=False)[1:], got)
        # the epilogue is flr_gru_bwd_step's math: the unfused kernel fed the fused dh_t gives the same bits
        assert_same_bits(BWD_NAMES, run_bwd_step(cuda, c, t - 1, dh0), got)
        if form in BW_SAME_ORDER:
            knob("FLR_GRU_BW", "8,2")
            assert_same_bits(("dh0",) + BWD_NAMES, [dh0] + got, run_bwd_fused(cuda, c, t))


# ---- 4. shared weights ------------------------------------------------------

SHARED = [(3, 5, 3, 24), (2, 32, 2, 300)]


def shared_case(shape):
    """The shape's case with client 0's W_hh given to every client; the other
    inputs (h_t, gi, gates, dgh, ...) stay per client."""
    c = case(shape)
    d = clients(c, c.K)
    d.whh = c.whh[:1].expand(c.K, -1, -1).contiguous()
    d.whhP = gru_ref.pack(d.whh, 3, c.H, c.H, 0)
    d.whhTP = gru_ref.pack(d.whh, 1, c.H, 3 * c.H, 1)
    return d


def device_pack(dev, w, NG, H, C, trans):
    """flr_gru_pack of w ([K, NG*H*C]) -> CPU [K, packed]."""
    K = w.shape[0]
    a = Arena(dev, w=w, wp=prefilled(K, _gru_packed(NG, H, C)))
    a.own("wp")
    _capi.call("flr_gru_pack", a.ptr("w"), K, NG, H, C, trans, a.ptr("wp"), stream())
    a.check()
    return a.get("wp")


@pytest.mark.parametrize("shape", SHARED, ids=_ids(SHARED))
def test_shared_weights_equal_replicated(cuda, shape):
    K, B, T, H = shape
    d = shared_case(shape)
    assert not torch.equal(d.h[0], d.h[1]) and not torch.equal(d.dgh[0], d.dgh[1])
    t = T - 1
    one = device_pack(cuda, d.whh[:1].reshape(1, -1), 3, H, H, 0)            # [1, packed]: the one copy
    rep = device_pack(cuda, d.whh.reshape(K, -1), 3, H, H, 0)
    got = run_fwd_fused(cuda, d, t, whhP=one, shared=1)
    assert_same_bits(FWD_NAMES, got, run_fwd_fused(cuda, d, t, whhP=rep, shared=0))
    for name, g, w in zip(FWD_NAMES, got, fwd_ref_of(d, t)):                 # every client from its own state
        assert_tensor(name, g, w)
    oneT = device_pack(cuda, d.whh[:1].reshape(1, -1), 1, H, 3 * H, 1)
    repT = device_pack(cuda, d.whh.reshape(K, -1), 1, H, 3 * H, 1)
    gotb = run_bwd_fused(cuda, d, t, whhTP=oneT, shared=1)
    assert_same_bits(("dh0",) + BWD_NAMES, gotb, run_bwd_fused(cuda, d, t, whhTP=repT, shared=0))
    for name, g, w in zip(("dh0",) + BWD_NAMES, gotb, bwd_ref_of(d, t)):
        assert_tensor(name, g, w)


# ---- 5. a client's result does not depend on the launch's client count --------

def test_client_count_invariance(cuda):
    shape = (8, 4, 2, 96)
    c8 = case(shape)          # grid 24: a multiple of 8, workgroups remapped
    c3 = clients(c8, 3)       # grid 9: not remapped
    f8, f3 = run_fwd_fused(cuda, c8, 1), run_fwd_fused(cuda, c3, 1)
    assert_same_bits(FWD_NAMES, [x[:3] for x in f8], f3)
    b8, b3 = run_bwd_fused(cuda, c8, 1), run_bwd_fused(cuda, c3, 1)
    assert_same_bits(("dh0",) + BWD_NAMES, [x[:3] for x in b8], b3)


# ---- 6. the unfused step kernels ----------------------------------------------

UNFUSED = [(2, 33, 3, 40), (3, 5, 2, 7)]   # B > 32; K B H = 105: one partial workgroup


@pytest.mark.parametrize("shape", UNFUSED, ids=_ids(UNFUSED))
def test_unfused_steps_vs_fp64(cuda, shape):
    c = case(shape)
    for t in sorted({0, c.T - 1}):
        got = run_fwd_step(cuda, c, t, c.gh)
        ref = fwd_ref_of(c, t, gh=c.gh)
        assert torch.equal(bits(got[3]), bits(c.gh[..., 2 * c.H:]))   # hn is a copy
        for name, g, w in zip(FWD_NAMES, got, ref):
            assert_tensor(name, g, w)
        gotb = run_bwd_step(cuda, c, t, c.dh)
        refb = bwd_ref_of(c, t + 1, dh_t=c.dh.double())[1:]
        for name, g, w in zip(BWD_NAMES, gotb, refb):
            assert_tensor(name, g, w)


# ---- 7. fused against batched GEMM + gate kernel ------------------------------

def test_fused_vs_unfused_forward(cuda):
    shape = (2, 32, 3, 40)
    c = case(shape)
    t = c.T - 1
    fused = run_fwd_fused(cuda, c, t)
    gh = bgemm(c.h[:, t].to(cuda), c.whh.to(cuda), bias=c.bhh.to(cuda)).cpu()
    unfused = run_fwd_step(cuda, c, t, gh)
    ref = fwd_ref_of(c, t)
    for name, f, u, w in zip(FWD_NAMES, fused, unfused, ref):
        assert_tensor(name + " fused", f, w)
        assert_tensor(name + " unfused", u, w)
        assert_tensor(name + " fused vs unfused", f, u.double(), factor=2.0)


# ---- a non-finite batch row stays in its row ----------------------------------

NAN_ROWS = [(3, 5, 3, 24), (3, 17, 3, 37)]


@pytest.mark.parametrize("shape", NAN_ROWS, ids=_ids(NAN_ROWS))
def test_nan_row_stays_in_its_row(cuda, shape):
    """The GEMM rows are batch rows: a NaN in row 1 of one client's A operand
    (h_t forward, dgh_t backward) makes that row's results NaN and leaves every
    other row's bits alone.  At H % 16 == 8 the last k-step's upper half lies
    past the row's end, where the next row starts: a load that reads it
    multiplies row 1's NaN into row 0 (the packed padding it meets is 0)."""
    K, B, T, H = shape
    c = case(shape)
    t = T - 1
    d = clients(c, K)
    d.h, d.dgh = c.h.clone(), c.dgh.clone()
    d.h[1, t, 1, 0] = float("nan")
    d.dgh[1, t, 1, 0] = float("nan")
    rows = [b for b in range(B) if b != 1]
    clean, dirty = run_fwd_fused(cuda, c, t), run_fwd_fused(cuda, d, t)
    assert torch.isnan(dirty[3][1, 1]).all()
    for name, x, y in zip(FWD_NAMES, clean, dirty):
        assert torch.equal(bits(x[:, rows]), bits(y[:, rows])) and torch.equal(bits(x[[0, 2]]), bits(y[[0, 2]])), name
    clean, dirty = run_bwd_fused(cuda, c, t), run_bwd_fused(cuda, d, t)
    assert torch.isnan(dirty[0][1, 1]).all()
    for name, x, y in zip(("dh0",) + BWD_NAMES, clean, dirty):
        assert torch.equal(bits(x[:, rows]), bits(y[:, rows])) and torch.equal(bits(x[[0, 2]]), bits(y[[0, 2]])), name


# ---- 8. rejected arguments ----------------------------------------------------

def _reject_arena(dev):
    K, B, T, H = 2, 32, 3, 8
    return (K, B, T, H), Arena(
        dev, gi=prefilled(K, B, T, 3 * H), gh=prefilled(K, B, 3 * H), whhP=prefilled(K, _gru_packed(3, H, H)),
        whhTP=prefilled(K, _gru_packed(1, H, 3 * H)), bhh=prefilled(K, 3 * H), hseq=prefilled(K, T + 1, B, H),
        gates=prefilled(K, T, B, 4, H), dgh=prefilled(K, T, B, 3 * H), dgi=prefilled(K, B, T, 3 * H),
        dhd=prefilled(K, B, H), dh0=prefilled(K, B, H), dh=prefilled(K, B, H), w=prefilled(K, 3 * H * H))


ENTRIES = {  # name -> (pointer arguments in order, the optional ones)
    "flr_gru_fwd_fused": (("gi", "whhP", "bhh", "hseq", "gates"), ()),
    "flr_gru_bwd_fused": (("whhTP", "gates", "hseq", "dgh", "dgi", "dhd", "dh0"), ("dh0",)),
    "flr_gru_fwd_step": (("gi", "gh", "hseq", "gates"), ()),
    "flr_gru_bwd_step": (("dh", "gates", "hseq", "dgh", "dgi", "dhd"), ()),
}


def _bad_calls():
    """(id, entry, {dimension overrides}, pointer to pass as NULL or None)."""
    out = []
    for e in ("flr_gru_fwd_fused", "flr_gru_bwd_fused"):
        out.append((f"{e}-B33", e, dict(B=33), None))
    out.append(("flr_gru_bwd_fused-t0", "flr_gru_bwd_fused", dict(t=0), None))
    for e, (ptrs, optional) in ENTRIES.items():
        out.append((f"{e}-tT", e, dict(t=3), None))
        out.append((f"{e}-K0", e, dict(K=0), None))
        out.append((f"{e}-H0", e, dict(H=0), None))
        out += [(f"{e}-null-{p}", e, {}, p) for p in ptrs if p not in optional]
    return out


BAD = _bad_calls()


@pytest.mark.parametrize("bad", BAD, ids=[b[0] for b in BAD])
def test_rejected_arguments(cuda, bad):
    _, entry, over, null = bad
    (K, B, T, H), a = _reject_arena(cuda)
    dims = dict(K=K, B=B, T=T, H=H, t=1)
    dims.update(over)
    ptrs = [None if p == null else a.ptr(p) for p in ENTRIES[entry][0]]
    rc = getattr(_capi.lib(), entry)(*ptrs, dims["K"], dims["B"], dims["T"], dims["H"], dims["t"], stream())
    assert rc == FLR_ERR_ARG
    a.check()   # nothing owned: every float of the arena holds its bits


@pytest.mark.parametrize("which", ["trans1-NG3", "null-w", "null-wp", "K0", "H0"])
def test_pack_rejected_arguments(cuda, which):
    (K, B, T, H), a = _reject_arena(cuda)
    args = dict(w=a.ptr("w"), K=K, NG=1, H=H, C=3 * H, trans=1, wp=a.ptr("whhTP"))
    args.update({"trans1-NG3": dict(NG=3, C=H), "null-w": dict(w=None), "null-wp": dict(wp=None), "K0": dict(K=0),
                 "H0": dict(H=0)}[which])
    rc = _capi.lib().flr_gru_pack(args["w"], args["K"], args["NG"], args["H"], args["C"], args["trans"], args["wp"],
                                  stream())
    assert rc == FLR_ERR_ARG
    a.check()
