"""Timing of the robust learning rate's kernels at C3's aggregate shape (K=128,
P = the default model's parameter count), all in one process on one matrix:
flr_rlr_fedavg (the vote fused into the FedAvg pass), flr_fedavg alone (the
yardstick: the same K*P*4 bytes), the three-call composition (flr_fedavg,
flr_sign_vote, flr_rlr_apply: two passes over the matrix) and flr_sign_vote
alone.  Event-timed on one stream: every kernel warmed up, then REPS rounds that
time the kernels in turn (N back-to-back calls per window), so drift over the
run hits all of them alike; the table gives each kernel's median window, its
min-max spread and the rate over the bytes the algorithm moves, next to the
fused call's byte floor (K*P + 3*P)*4 over the HBM rate.  The fused kernel is
worth keeping only if it beats the composition by more than that spread.
Env: K, P, N (calls per window), REPS, THETA."""
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-fl-security_amd"))
import torch
from flr import ops
from flr.models.multimodal import ModelSpec, num_params
from flr.workload import update_matrix

HBM_TBS = 8.0  # the MI355X's peak HBM rate, TB/s
K = int(os.environ.get("K", 128))
P = int(os.environ.get("P", 0)) or num_params(ModelSpec())
N = int(os.environ.get("N", 30)); REPS = int(os.environ.get("REPS", 5))
THETA = int(os.environ.get("THETA", max(1, round(0.7 * K ** 0.5))))  # some coordinates pass, some flip
assert torch.cuda.is_available(), "robust_lr_bench needs a GPU"
X = update_matrix(K, P, f=0, device="cuda")[:, :P]
n = torch.arange(1, K + 1, dtype=torch.int64, device="cuda")
g = ops.fedavg(X, torch.ones_like(n))  # the rows' mean: votes of about sqrt(K) either way
out = torch.empty(P, device="cuda"); agg = torch.empty(P, device="cuda")
votes = torch.empty(P, dtype=torch.int32, device="cuda")
def composed():
    ops.fedavg(X, n, out=agg)
    ops.sign_vote(X, g, out=votes)
    ops.rlr_apply(agg, g, votes, THETA, 1.0, out=agg, count=True)
kp, p4 = 4 * K * P, 4 * P
kernels = [  # name, call, bytes moved
    ("rlr_fedavg (fused)", lambda: ops.rlr_fedavg(X, n, g, THETA, 1.0, out=out), kp + 2 * p4),
    ("rlr_fedavg + votes, flipped", lambda: ops.rlr_fedavg(X, n, g, THETA, 1.0, out=out, diagnostics=True), kp + 3 * p4),
    ("fedavg", lambda: ops.fedavg(X, n, out=agg), kp + p4),
    ("fedavg, sign_vote, rlr_apply", composed, 2 * kp + 7 * p4),
    ("sign_vote", lambda: ops.sign_vote(X, g, out=votes), kp + 2 * p4),
]
def window(fn):
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(N): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / N
for _, fn, _ in kernels:
    for _ in range(3): fn()
torch.cuda.synchronize()
# the fused call and the composition: the same bits, at the size that is timed
o1, v1, f1 = ops.rlr_fedavg(X, n, g, THETA, 1.0, diagnostics=True)
o2, f2 = ops.rlr_apply(ops.fedavg(X, n), g, ops.sign_vote(X, g), THETA, 1.0, count=True)
assert torch.equal(o1.view(torch.int32), o2.view(torch.int32)) and f1.item() == f2.item()
times = {name: [] for name, _, _ in kernels}
for _ in range(REPS):
    for name, fn, _ in kernels:
        times[name].append(window(fn))
floor = (K * P + 3 * P) * 4 / (HBM_TBS * 1e12) * 1e3
print(f"K={K} P={P} theta={THETA}: K*P*4 = {kp / 1e9:.3f} GB, {f1.item()} of {P} coordinates flipped, "
      f"{N} calls per window, {REPS} windows per kernel; byte floor of the fused call (K*P + 3*P)*4 / "
      f"{HBM_TBS:g} TB/s = {floor:.3f} ms", flush=True)
print("| call | median ms | min | max | GB moved | TB/s |\n|---|---|---|---|---|---|")
for name, _, nbytes in kernels:
    t = statistics.median(times[name])
    print(f"| {name} | {t:.3f} | {min(times[name]):.3f} | {max(times[name]):.3f} | {nbytes / 1e9:.3f} | "
          f"{nbytes / t / 1e9:.2f} |", flush=True)
