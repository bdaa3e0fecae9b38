"""GPU: flr_train_clients (the client plugin as one C entry, SURVEY §8(b);
FLClient.fit / _train fl_client.py:76-149, run_experiments.py:193-240) gives
the bits of the Python trainer (ClientBatchTrainer: the same kernels driven
through torch autograd) — trained rows, per-client mean loss and clip norms —
and the reference loop (the oracle) at 1e-5."""
import pytest
import torch

from oracle import training as otrain
from parity import check_conditioned, check_delta, conditioned_report, delta_report, gate_ties, record
from flr import native_trainer as nt
from flr.models.multimodal import TINY, ModelSpec, MultimodalNet, param_layout
from flr.round import initial_global
from flr.train import ClientBatchTrainer, TrainConfig, make_dropout_masks, synthetic_batches

pytestmark = pytest.mark.gpu


# c3_b128: batch 128 gives the 128 x 128 weight-gradient tiles a deeper split-K
# than the smaller tiles (the workspace and the fused clip-norm slots
# must follow the tile the launch takes)
# c3_overlap: the optimizer update on the side stream under the next step's forward
# (FLR_SGD_OVERLAP=1, side_stream.h), three steps so two updates overlap a forward
# c3_b32: batch 32 takes the fused stem BN + ReLU + max-pool kernels (flr_batchnorm_relu_maxpool_fwd / _bwd)
@pytest.mark.parametrize("spec_name,B,nneg", [("tiny", 4, 1), ("c3", 8, 1), ("c3_b32", 32, 1), ("c3_b40", 40, 0),
                                              ("c3_b128", 128, 0), ("c3_overlap", 8, 1)])
def test_native_trainer_bit_identical_to_python_trainer(cuda, spec_name, B, nneg, knob):
    spec = TINY if spec_name == "tiny" else ModelSpec()
    K, steps = 3, 2
    if spec_name == "c3_overlap":
        from flr import _capi
        if "ablation" not in _capi.build_info():
            pytest.skip("the side-stream optimizer is a tools-build form (make ABLATION=1)")
        knob("FLR_SGD_OVERLAP", "1")
        steps = 3
    cfg = TrainConfig(local_steps=steps)
    glob = initial_global(spec, 42, cuda)
    batches = synthetic_batches(spec, steps, range(K), B, cuda)
    masks = make_dropout_masks(spec, steps, K, B, cuda, seed=11)
    tr = ClientBatchTrainer(spec, K, cuda, cfg)
    tr.load_global(glob)
    loss_py = tr.local_update(batches, masks, negate_rows=nneg).clone()
    X_py = tr.X.data[:, : tr.P].clone()
    norms_py = tr.norms.clone()
    X, loss, norms = nt.train_clients(spec, glob, batches, cfg, masks, negate_rows=nneg)
    torch.cuda.synchronize()
    assert torch.isfinite(X).all()
    assert torch.equal(loss, loss_py), (loss, loss_py)
    assert torch.equal(norms, norms_py), (norms, norms_py)
    assert torch.equal(X, X_py), (X - X_py).abs().max()


@pytest.fixture(scope="module")
def c3_default_streams(cuda):
    """flr_train_clients on the full ResNet-18 + GRU model (tap-major convs, the
    three downsample blocks, the two blocks whose weight gradients go to the text
    stream) with every auxiliary stream at its default: the inputs and the result."""
    spec, K, B, steps = ModelSpec(), 3, 8, 2
    cfg = TrainConfig(local_steps=steps)
    glob = initial_global(spec, 42, cuda)
    batches = synthetic_batches(spec, steps, range(K), B, cuda)
    masks = make_dropout_masks(spec, steps, K, B, cuda, seed=11)
    X, loss, norms = nt.train_clients(spec, glob, batches, cfg, masks, negate_rows=1)
    torch.cuda.synchronize()
    return (spec, glob, batches, cfg, masks), (X, loss, norms)


# where the work runs changes no bit: the text branch, the weight gradients and the
# shortcut convs on the caller's stream instead of their own (the gates are read per call)
@pytest.mark.parametrize("off", [("FLR_TEXT_STREAM",), ("FLR_WGRAD_STREAM",), ("FLR_TEXT_STREAM", "FLR_WGRAD_STREAM"),
                                 ("FLR_WG_TEXT",)], ids="+".join)
def test_native_trainer_same_bits_on_any_stream(c3_default_streams, knob, off):
    (spec, glob, batches, cfg, masks), (X0, loss0, norms0) = c3_default_streams
    for name in off:
        knob(name, "0")
    X, loss, norms = nt.train_clients(spec, glob, batches, cfg, masks, negate_rows=1)
    torch.cuda.synchronize()
    assert torch.equal(X, X0), (X - X0).abs().max()
    assert torch.equal(loss, loss0), (loss, loss0)
    assert torch.equal(norms, norms0), (norms, norms0)


def _gpu_relu_inputs(spec, w, images, tokens, mask, cuda):
    """The ReLU inputs of one train-mode forward of the engine's kernels (the
    Python trainer's composition, bit-identical to flr_train_clients:
    test_native_trainer_bit_identical_to_python_trainer) from the flat
    parameters w, as [B, C, H, W] per fused BatchNorm + ReLU, in call order."""
    from flr.models import multimodal as mm
    from flr.nn import client_batchnorm
    rec, orig = [], mm._bn_act

    def bn_act(x, g, b, residual=None, relu=True, stats=None):
        if relu and stats is None:
            z = client_batchnorm(x, g, b, residual, relu=False)
            rec.append(z.detach().view(g.numel(), *z.shape[1:]).transpose(0, 1).cpu())
        return orig(x, g, b, residual, relu, stats)

    tr = ClientBatchTrainer(spec, 1, cuda, TrainConfig(local_steps=1))
    tr.load_global(w)
    params = dict(zip(tr.names, [t.detach() for t in tr.W]))
    mm._bn_act = bn_act
    try:
        with torch.no_grad():
            mm.batched_forward(params, images, tokens, spec, mask, tr.tap_major, tr.skip_dead)
    finally:
        mm._bn_act = orig
    torch.cuda.synchronize()
    return rec


def test_native_trainer_matches_reference_loop(cuda):
    """Two local steps of the full ResNet-18 + GRU model at the bench's batch of 32
    against the reference loop: whole vector 1e-5 after both steps; per tensor
    (tests/parity.py) after the first step, for every client.  Step 2 is asserted
    per tensor as a STEP, from the GPU's own step-1 state, for every client: the
    GPU's second step against the reference's second step from that state,
    within 4x the reference's own distance from the same step in fp64 plus 1e-5
    of the update (tests/parity.py check_conditioned).
    Client 0 of this data set meets a ReLU gate at layers.1.0's output whose fp64
    pre-activation (-7.1e-7, std 1.41) lies inside fp32 rounding of zero: the
    reference's fp32 sums land below zero, the GPU's above — with its bf16x6
    conv products and with exact-fp32 MFMA products alike (tools/diag_gate_prec.py,
    profiles/r6_records/diag_gate_prec_B32_k0.json): a summation-order tie, not
    a precision loss.  Both reference runs therefore take the engine's decision at
    such ties (parity.gate_ties: each must lie within 4x the reference's own RMS
    fp32 rounding of that layer, at most 8 per forward; the record lists them);
    every other decision and every operation is the reference's."""
    spec = ModelSpec()
    K, B, steps = 2, 32, 2
    glob = initial_global(spec, 42, cuda)
    batches = synthetic_batches(spec, steps, range(K), B, cuda)
    masks = make_dropout_masks(spec, steps, K, B, cuda, seed=3)
    payload = {"config": "flr_train_clients, ResNet-18 + GRU, K=2, B=32, dropout masks"}
    w1, step2, step2c, cond, tie_rep = {}, {}, {}, {}, {}
    for nst in (1, 2):
        X, loss, _ = nt.train_clients(spec, glob, batches[:nst], TrainConfig(local_steps=nst), masks[:nst])
        reps = {}
        for k in range(K):
            cb = [(im[k].cpu(), tk[k].cpu(), lb[k].cpu()) for im, tk, lb in batches[:nst]]
            upd, ref_loss = otrain.local_update(MultimodalNet, spec, glob.cpu(), cb,
                                                masks=[m[k].cpu() for m in masks[:nst]])
            ref = torch.cat([u.reshape(-1) for u in upd])
            err = ((X[k].cpu().double() - ref.double()).abs().max() / ref.abs().max()).item()
            assert err < 1e-5, (nst, k, err)
            assert abs(loss[k].item() - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
            reps[f"client{k}"] = delta_report(X[k], ref, glob, param_layout(spec))
            if nst == 1:
                w1[k] = X[k].clone()
            else:
                # step 2 of the reference FROM THE GPU'S OWN STEP-1 STATE (its
                # weights; the reference's step-1 momentum, equal to the GPU's
                # clipped gradient within fp32 noise), with the gate ties resolved
                # as the engine resolved them; and the conditioning, recorded: how
                # far the fp32 reference's own step 2 moves when its step-1 state
                # is replaced by the GPU's (the step-1 states agree to fp32 noise)
                im2, tk2, _ = cb[1]
                zg = _gpu_relu_inputs(spec, w1[k], batches[1][0][k:k + 1], batches[1][1][k:k + 1],
                                      masks[1][k:k + 1], cuda)
                z32 = otrain.relu_inputs(MultimodalNet, spec, w1[k].cpu(), im2, tk2)
                z64 = otrain.relu_inputs(MultimodalNet, spec, w1[k].cpu(), im2, tk2, dtype=torch.float64)
                ties, tie_rep[f"client{k}"] = gate_ties(zg, z32, z64)
                _, _, buf1 = otrain.local_update(MultimodalNet, spec, glob.cpu(), cb[:1], masks=[masks[0][k].cpu()],
                                                 return_momentum=True)
                upd_h, _ = otrain.local_update(MultimodalNet, spec, glob.cpu(), cb[1:], masks=[masks[1][k].cpu()],
                                               start_params=w1[k].cpu(), start_momentum=buf1, relu_ties=ties)
                ref_h = torch.cat([u.reshape(-1) for u in upd_h])
                upd_h64, _ = otrain.local_update(MultimodalNet, spec, glob.cpu(), cb[1:], masks=[masks[1][k].cpu()],
                                                 start_params=w1[k].cpu(), start_momentum=buf1, dtype=torch.float64,
                                                 relu_ties=ties)
                ref_h64 = torch.cat([u.reshape(-1) for u in upd_h64])
                step2[f"client{k}"] = delta_report(X[k], ref_h, w1[k], param_layout(spec))
                step2c[f"client{k}"] = conditioned_report(X[k], ref_h, ref_h64, w1[k], param_layout(spec))
                cond[f"client{k}"] = delta_report(ref_h, ref, w1[k], param_layout(spec))
        payload[f"steps{nst}"] = reps
        if nst == 1:
            check_delta(reps)
    payload["step2_gate_ties"] = tie_rep
    payload["step2_from_gpu_state"] = step2
    payload["step2_from_gpu_state_conditioned"] = step2c
    payload["step2_reference_conditioning"] = cond
    record("native_resnet_gru_update_parity.json", payload)
    # step 2 from the same state, every client: per tensor within 4x the fp32
    # reference's own distance from the fp64 step (+ 1e-5 of the update)
    check_conditioned(step2c)


def _vit_python(spec, glob, batches, masks, K, steps, chunk, nneg, cuda):
    tr = ClientBatchTrainer(spec, K, cuda, TrainConfig(local_steps=steps, client_chunk=chunk))
    tr.load_global(glob)
    loss = tr.local_update(batches, masks, negate_rows=nneg).clone()
    return loss, tr.X.data[:, : tr.P].clone(), tr.norms.clone()


# flr_train_vit_bert (the C4/C5 family's one-call trainer) vs the Python
# trainer: the same kernels driven through torch autograd, the same bits.
# tiny: ragged client passes (chunk 2 of K 3); full: the ViT-S/4 + BERT-mini
# model itself with dropout masks, attackers negated
@pytest.mark.parametrize("spec_name,K,B,steps,chunk,nneg", [("vit_tiny", 3, 4, 2, 2, 1), ("vit_tiny_b32", 2, 32, 1, 0, 0),
                                                            ("vit_full", 2, 4, 2, 0, 1)])
def test_native_vit_bert_bit_identical_to_python_trainer(cuda, spec_name, K, B, steps, chunk, nneg):
    from flr.models.multimodal import VIT_BERT, VIT_BERT_TINY
    spec = VIT_BERT if spec_name == "vit_full" else VIT_BERT_TINY.__class__(**{**VIT_BERT_TINY.__dict__,
                                                                              "dropout": 0.5})
    glob = initial_global(spec, 42, cuda)
    batches = synthetic_batches(spec, steps, range(K), B, cuda)
    masks = make_dropout_masks(spec, steps, K, B, cuda, seed=5)
    loss_py, X_py, norms_py = _vit_python(spec, glob, batches, masks, K, steps, chunk, nneg, cuda)
    tr = nt.NativeRoundTrainer(spec, K, cuda, TrainConfig(local_steps=steps, client_chunk=chunk), batch=B)
    assert tr.chunks == ClientBatchTrainer(spec, K, cuda, TrainConfig(local_steps=steps, client_chunk=chunk)).chunks
    tr.load_global(glob)
    loss = tr.local_update(batches, masks, negate_rows=nneg)
    torch.cuda.synchronize()
    X = tr.X.data[:, : tr.P]
    assert torch.isfinite(X).all()
    assert torch.equal(loss, loss_py), (loss, loss_py)
    assert torch.equal(tr.norms, norms_py), (tr.norms, norms_py)
    assert torch.equal(X, X_py), (X - X_py).abs().max()


def test_native_vit_bert_same_bits_without_wgrad_stream(cuda, knob):
    """The vit_tiny case with the layers' weight / bias gradients on the caller's
    stream (FLR_WGRAD_STREAM=0, read per call) and on their own: the same bits."""
    from flr.models.multimodal import VIT_BERT_TINY
    spec = VIT_BERT_TINY.__class__(**{**VIT_BERT_TINY.__dict__, "dropout": 0.5})
    K, B, steps, chunk, nneg = 3, 4, 2, 2, 1
    glob = initial_global(spec, 42, cuda)
    batches = synthetic_batches(spec, steps, range(K), B, cuda)
    masks = make_dropout_masks(spec, steps, K, B, cuda, seed=5)
    got = []
    for value in ("0", None):
        knob("FLR_WGRAD_STREAM", value)
        tr = nt.NativeRoundTrainer(spec, K, cuda, TrainConfig(local_steps=steps, client_chunk=chunk), batch=B)
        tr.load_global(glob)
        loss = tr.local_update(batches, masks, negate_rows=nneg).clone()
        torch.cuda.synchronize()
        got.append((tr.X.data[:, : tr.P].clone(), loss, tr.norms.clone()))
    (X0, loss0, norms0), (X1, loss1, norms1) = got
    assert torch.isfinite(X1).all()
    assert torch.equal(X0, X1), (X0 - X1).abs().max()
    assert torch.equal(loss0, loss1), (loss0, loss1)
    assert torch.equal(norms0, norms1), (norms0, norms1)


def test_native_vit_bert_matches_reference_loop(cuda):
    """flr_train_vit_bert vs the oracle loop on one ViTBertNet per client (1e-5)."""
    from flr.models.multimodal import VIT_BERT_TINY, model_class
    spec = VIT_BERT_TINY.__class__(**{**VIT_BERT_TINY.__dict__, "dropout": 0.5})
    K, B, steps = 3, 8, 3
    glob = initial_global(spec, 42, cuda)
    batches = synthetic_batches(spec, steps, range(K), B, cuda)
    masks = make_dropout_masks(spec, steps, K, B, cuda, seed=4)
    tr = nt.NativeRoundTrainer(spec, K, cuda, TrainConfig(local_steps=steps), batch=B)
    tr.load_global(glob)
    loss = tr.local_update(batches, masks).cpu()
    reps = {}
    for k in range(K):
        cb = [(im[k].cpu(), tk[k].cpu(), lb[k].cpu()) for im, tk, lb in batches]
        upd, ref_loss = otrain.local_update(model_class(spec), spec, glob.cpu(), cb, masks=[m[k].cpu() for m in masks])
        ref = torch.cat([u.reshape(-1) for u in upd])
        got = tr.X.data[k, : tr.P].cpu()
        err = ((got.double() - ref.double()).abs().max() / ref.abs().max()).item()
        assert err < 1e-5, err
        assert abs(loss[k].item() - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
        reps[f"client{k}"] = delta_report(got, ref, glob, param_layout(spec))
    record("native_vit_bert_tiny_update_parity.json",
           {"config": "flr_train_vit_bert, ViT/BERT tiny, K=3, B=8, 3 steps, dropout masks", **reps})
    check_delta(reps)
