"""a3: the one-launch GRU recurrence (flr_gru_fwd_seq / flr_gru_bwd_seq) against
the per-step C entries run over the same inputs.  Every comparison is of int32
views: the one-launch form claims the per-step default form's bits.

The buffers of a run are slices of one arena (test_gpu_gru_steps.Arena) with
NaN margins; outputs are prefilled with another NaN pattern, so every run also
checks that nothing outside the slots it owns changed and that every owned
slot was written."""
import dataclasses

import pytest
import torch

from flr import _capi
from test_gpu_gru_steps import (Arena, assert_same_bits, bits, case, clients, device_pack, only_slot, prefilled,
                                shared_case, stream)

pytestmark = pytest.mark.gpu

SHAPES = [  # (K, B, T, H)
    (1, 1, 1, 32),     # the backward has no GEMM step; one wave
    (2, 5, 2, 32),
    (3, 32, 3, 64),
    (2, 17, 4, 96),    # S = 6: two of the eight k-ranges empty; B crosses 16
    (8, 4, 2, 96),
    (2, 32, 3, 256),   # the workload's H at small K and T
]
FLR_ERR_ARG, FLR_ERR_UNSUPPORTED = -1, -3
FWD_OUT = ("hseq", "gates")
BWD_OUT = ("dgh", "dgi", "dh_direct", "dh0")


def _ids(xs):
    return [str(x).replace(" ", "") for x in xs]


def fwd_arena(dev, c, whhP=None):
    a = Arena(dev, whhP=c.whhP if whhP is None else whhP, gi=c.gi, bhh=c.bhh, hseq=only_slot(c.h, 1, 0),
              gates=prefilled(c.K, c.T, c.B, 4, c.H))
    a.own("hseq", slice(None), slice(1, None))
    a.own("gates")
    return a


def run_fwd(dev, c, seq, whhP=None, shared=0):
    """The whole forward from hseq[:, 0] = c.h[:, 0]: one flr_gru_fwd_seq call, or
    flr_gru_fwd_fused_ex for t = 0 .. T-1.  Returns (hseq, gates) as written."""
    K, B, T, H = c.K, c.B, c.T, c.H
    a = fwd_arena(dev, c, whhP)
    if seq:
        _capi.call("flr_gru_fwd_seq", a.ptr("gi"), a.ptr("whhP"), shared, a.ptr("bhh"), a.ptr("hseq"), a.ptr("gates"),
                   K, B, T, H, stream())
    else:
        for t in range(T):
            _capi.call("flr_gru_fwd_fused_ex", a.ptr("gi"), a.ptr("whhP"), shared, a.ptr("bhh"), a.ptr("hseq"),
                       a.ptr("gates"), K, B, T, H, t, stream())
    a.check()
    return a.get("hseq"), a.get("gates")


def bwd_arena(dev, c, whhTP=None):
    K, B, T, H = c.K, c.B, c.T, c.H
    a = Arena(dev, whhTP=c.whhTP if whhTP is None else whhTP, gates=c.gates, hseq=c.h, dh=c.dh,
              dgh=prefilled(K, T, B, 3 * H), dgi=prefilled(K, B, T, 3 * H), dhd=prefilled(K, B, H),
              dh0=prefilled(K, B, H))
    a.own("dgh")
    a.own("dgi")
    a.own("dhd")
    if T >= 2:          # dh0 is the t = 1 step's: no such step at T = 1
        a.own("dh0")
    return a


def run_bwd(dev, c, seq, whhTP=None, shared=0, with_dh0=True):
    """The whole backward from dh = dL/dh_T: one flr_gru_bwd_seq call, or
    flr_gru_bwd_step at T-1 and flr_gru_bwd_fused_ex for t = T-1 .. 1 (dh0 given
    to the t = 1 call).  Returns (dgh, dgi, dh_direct, dh0)."""
    K, B, T, H = c.K, c.B, c.T, c.H
    a = bwd_arena(dev, c, whhTP)
    if not with_dh0:
        a.owned[a.span["dh0"][0]:a.span["dh0"][0] + K * B * H] = False
    dh0 = a.ptr("dh0") if with_dh0 else None
    if seq:
        _capi.call("flr_gru_bwd_seq", a.ptr("whhTP"), shared, a.ptr("gates"), a.ptr("hseq"), a.ptr("dh"),
                   a.ptr("dgh"), a.ptr("dgi"), a.ptr("dhd"), dh0, K, B, T, H, stream())
    else:
        _capi.call("flr_gru_bwd_step", a.ptr("dh"), a.ptr("gates"), a.ptr("hseq"), a.ptr("dgh"), a.ptr("dgi"),
                   a.ptr("dhd"), K, B, T, H, T - 1, stream())
        for t in range(T - 1, 0, -1):
            _capi.call("flr_gru_bwd_fused_ex", a.ptr("whhTP"), shared, a.ptr("gates"), a.ptr("hseq"), a.ptr("dgh"),
                       a.ptr("dgi"), a.ptr("dhd"), dh0 if t == 1 else None, K, B, T, H, t, stream())
    a.check()
    return a.get("dgh"), a.get("dgi"), a.get("dhd"), a.get("dh0")


# ---- 1. the per-step bits, every owned slot written, nothing else touched ----

@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_fwd_seq_is_the_per_step_bits(cuda, shape):
    c = case(shape)
    assert _capi.lib().flr_gru_seq_supported(*shape) == 1
    assert_same_bits(FWD_OUT, run_fwd(cuda, c, True), run_fwd(cuda, c, False))


@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_bwd_seq_is_the_per_step_bits(cuda, shape):
    c = case(shape)
    got = run_bwd(cuda, c, True)
    assert_same_bits(BWD_OUT, got, run_bwd(cuda, c, False))
    # dh0 is optional: without it the rest is the same and dh0 keeps its bits
    assert_same_bits(BWD_OUT[:3], run_bwd(cuda, c, True, with_dh0=False)[:3], got[:3])


# ---- 2. shared weights, client count, a NaN row --------------------------------

def test_shared_weights_equal_replicated(cuda):
    shape = (3, 32, 3, 64)
    K, B, T, H = shape
    d = shared_case(shape)
    one = device_pack(cuda, d.whh[:1].reshape(1, -1), 3, H, H, 0)
    rep = device_pack(cuda, d.whh.reshape(K, -1), 3, H, H, 0)
    got = run_fwd(cuda, d, True, whhP=one, shared=1)
    assert_same_bits(FWD_OUT, got, run_fwd(cuda, d, True, whhP=rep, shared=0))
    assert_same_bits(FWD_OUT, got, run_fwd(cuda, d, False, whhP=one, shared=1))
    oneT = device_pack(cuda, d.whh[:1].reshape(1, -1), 1, H, 3 * H, 1)
    repT = device_pack(cuda, d.whh.reshape(K, -1), 1, H, 3 * H, 1)
    gotb = run_bwd(cuda, d, True, whhTP=oneT, shared=1)
    assert_same_bits(BWD_OUT, gotb, run_bwd(cuda, d, True, whhTP=repT, shared=0))
    assert_same_bits(BWD_OUT, gotb, run_bwd(cuda, d, False, whhTP=oneT, shared=1))


def test_client_count_invariance(cuda):
    c3 = case((3, 32, 3, 64))
    c1 = clients(c3, 1)
    assert_same_bits(FWD_OUT, [x[:1] for x in run_fwd(cuda, c3, True)], run_fwd(cuda, c1, True))
    assert_same_bits(BWD_OUT, [x[:1] for x in run_bwd(cuda, c3, True)], run_bwd(cuda, c1, True))


def test_nan_row_stays_in_its_row(cuda):
    """A NaN in batch row 1 of client 1 (h_0 forward; dh backward) reaches every
    step of that row and no other row or client."""
    shape = (3, 32, 3, 64)
    K, B, T, H = shape
    c = case(shape)
    d = clients(c, K)
    d.h, d.dh = c.h.clone(), c.dh.clone()
    d.h[1, 0, 1, 0] = float("nan")
    d.dh[1, 1, :] = float("nan")      # the whole row: step T-1 has no GEMM to spread one element
    rows = [b for b in range(B) if b != 1]
    clean, dirty = run_fwd(cuda, c, True), run_fwd(cuda, d, True)
    assert torch.isnan(dirty[0][1, 1:, 1]).all()          # hseq[k=1, t>=1, b=1]
    assert torch.equal(bits(clean[0][:, :, rows]), bits(dirty[0][:, :, rows]))
    assert torch.equal(bits(clean[1][:, :, rows]), bits(dirty[1][:, :, rows]))
    for x, y in zip(clean, dirty):
        assert torch.equal(bits(x[[0, 2]]), bits(y[[0, 2]]))
    # the backward reads gates / hseq as given (finite): the NaN enters through dh only
    cb = clients(c, K)
    cb.dh = d.dh
    clean, dirty = run_bwd(cuda, c, True), run_bwd(cuda, cb, True)
    assert torch.isnan(dirty[0][1, :, 1]).all() and torch.isnan(dirty[3][1, 1]).all()
    for name, x, y in zip(BWD_OUT, clean, dirty):
        bdim = 1 if name == "dgi" else (2 if name == "dgh" else 1)
        idx = [slice(None)] * x.dim()
        idx[bdim] = rows
        assert torch.equal(bits(x[tuple(idx)]), bits(y[tuple(idx)])), name
        assert torch.equal(bits(x[[0, 2]]), bits(y[[0, 2]])), name


# ---- 3. shapes the form does not take, and the knob ----------------------------

def _refused(dev, c):
    """Both entries answer FLR_ERR_UNSUPPORTED and write nothing."""
    K, B, T, H = c.K, c.B, c.T, c.H
    assert _capi.lib().flr_gru_seq_supported(K, B, T, H) == 0
    a = fwd_arena(dev, c)
    a.owned[:] = False
    rc = _capi.lib().flr_gru_fwd_seq(a.ptr("gi"), a.ptr("whhP"), 0, a.ptr("bhh"), a.ptr("hseq"), a.ptr("gates"),
                                     K, B, T, H, stream())
    assert rc == FLR_ERR_UNSUPPORTED
    a.check()
    a = bwd_arena(dev, c)
    a.owned[:] = False
    rc = _capi.lib().flr_gru_bwd_seq(a.ptr("whhTP"), 0, a.ptr("gates"), a.ptr("hseq"), a.ptr("dh"), a.ptr("dgh"),
                                     a.ptr("dgi"), a.ptr("dhd"), a.ptr("dh0"), K, B, T, H, stream())
    assert rc == FLR_ERR_UNSUPPORTED
    a.check()


@pytest.mark.parametrize("shape", [(2, 32, 3, 40), (2, 32, 2, 300)], ids=["H40", "H300"])
def test_ineligible_shapes_are_refused(cuda, shape):
    _refused(cuda, case(shape))


def test_batch_above_32_is_refused(cuda):
    _refused(cuda, case((2, 33, 3, 40)))


def test_knob_off_is_refused_and_per_step_holds(cuda, knob):
    shape = (2, 5, 2, 32)
    c = case(shape)
    on = run_fwd(cuda, c, True), run_bwd(cuda, c, True)
    knob("FLR_GRU_SEQ", "0")
    _refused(cuda, c)
    assert_same_bits(FWD_OUT, run_fwd(cuda, c, False), on[0])     # what the caller falls back to
    assert_same_bits(BWD_OUT, run_bwd(cuda, c, False), on[1])
    assert _capi.lib().flr_gru_seq_preferred(128, 32, 16, 256) == 0
    knob("FLR_GRU_SEQ", "1")
    assert _capi.lib().flr_gru_seq_supported(*shape) == 1
    assert _capi.lib().flr_gru_seq_preferred(*shape) == 1          # forced on below the K it pays from
    knob("FLR_GRU_SEQ", None)
    lib = _capi.lib()
    assert lib.flr_gru_seq_preferred(*shape) == 0 and lib.flr_gru_seq_preferred(128, 32, 16, 256) == 1
    assert lib.flr_gru_seq_preferred(96, 32, 16, 256) == 0 and lib.flr_gru_seq_preferred(128, 32, 16, 300) == 0


# ---- 4. rejected arguments -------------------------------------------------------

FWD_PTRS = ("gi", "whhP", "bhh", "hseq", "gates")
BWD_PTRS = ("whhTP", "gates", "hseq", "dh", "dgh", "dgi", "dhd", "dh0")


def _bad():
    out = [("fwd-T0", "fwd", dict(T=0), None), ("bwd-T0", "bwd", dict(T=0), None),
           ("fwd-K0", "fwd", dict(K=0), None), ("bwd-H0", "bwd", dict(H=0), None)]
    out += [(f"fwd-null-{p}", "fwd", {}, p) for p in FWD_PTRS]
    out += [(f"bwd-null-{p}", "bwd", {}, p) for p in BWD_PTRS if p != "dh0"]
    return out


BAD = _bad()


@pytest.mark.parametrize("bad", BAD, ids=[b[0] for b in BAD])
def test_rejected_arguments(cuda, bad):
    _, which, over, null = bad
    c = case((2, 5, 2, 32))
    dims = dict(K=c.K, B=c.B, T=c.T, H=c.H)
    dims.update(over)
    a = fwd_arena(cuda, c) if which == "fwd" else bwd_arena(cuda, c)
    a.owned[:] = False
    p = lambda n: None if n == null else a.ptr(n)  # noqa: E731
    if which == "fwd":
        rc = _capi.lib().flr_gru_fwd_seq(p("gi"), p("whhP"), 0, p("bhh"), p("hseq"), p("gates"), dims["K"], dims["B"],
                                         dims["T"], dims["H"], stream())
    else:
        rc = _capi.lib().flr_gru_bwd_seq(p("whhTP"), 0, p("gates"), p("hseq"), p("dh"), p("dgh"), p("dgi"), p("dhd"),
                                         p("dh0"), dims["K"], dims["B"], dims["T"], dims["H"], stream())
    assert rc == FLR_ERR_ARG
    a.check()


# ---- 5. the h_0 fill ---------------------------------------------------------------

def test_zero_h0_writes_slot_0_only(cuda):
    K, B, T, H = 3, 5, 2, 37
    a = Arena(cuda, hseq=prefilled(K, T + 1, B, H))
    a.own("hseq", slice(None), 0)
    _capi.call("flr_gru_zero_h0", a.ptr("hseq"), K, B, T, H, stream())
    a.check()
    assert torch.equal(bits(a.get("hseq")[:, 0]), torch.zeros(K, B, H, dtype=torch.int32))
    assert _capi.lib().flr_gru_zero_h0(None, K, B, T, H, stream()) == FLR_ERR_ARG
    assert _capi.lib().flr_gru_zero_h0(a.ptr("hseq"), K, B, 0, H, stream()) == FLR_ERR_ARG


# ---- 6. the native trainer takes the form, with the per-step trainer's bits ---------

@pytest.mark.parametrize("spec_name,B", [("tiny_h32", 4), ("c3", 8)])
def test_trainer_bits_with_and_without_the_form(cuda, knob, spec_name, B):
    from flr import native_trainer as nt
    from flr.models.multimodal import TINY, ModelSpec
    from flr.round import initial_global
    from flr.train import TrainConfig, make_dropout_masks, synthetic_batches
    # TINY's 16 hidden units are not a whole unit block; c3 is the workload's model (H = 256)
    spec = dataclasses.replace(TINY, hidden=32) if spec_name == "tiny_h32" else ModelSpec()
    K, steps = 3, 2                                     # step 1 shares the packed global W_hh, step 2 does not
    assert _capi.lib().flr_gru_seq_supported(K, B, spec.seq_len, spec.hidden) == 1
    cfg = TrainConfig(local_steps=steps)
    glob = initial_global(spec, 42, cuda)
    batches = synthetic_batches(spec, steps, range(K), B, cuda)
    masks = make_dropout_masks(spec, steps, K, B, cuda, seed=11)
    out = {}
    for on in ("0", "1"):
        knob("FLR_GRU_SEQ", on)
        tr = nt.NativeRoundTrainer(spec, K, cuda, cfg, batch=B)      # flr_train_clients_ex
        tr.load_global(glob)
        loss = tr.local_update(batches, masks, negate_rows=1)
        torch.cuda.synchronize()
        out[on] = (tr.X.data[:, : tr.P].clone(), loss.clone(), tr.norms.clone())
    assert torch.isfinite(out["1"][0]).all()
    for name, x, y in zip(("X", "loss", "norms"), out["0"], out["1"]):
        assert torch.equal(bits(x), bits(y)), name
