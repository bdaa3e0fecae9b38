"""Timing of SparseFed's calls at C3's aggregate shape (K=128, P = the default
model's parameter count), all in one process on one matrix: flr_row_norms,
flr_sparsefed_weights, flr_sparsefed_accumulate (momentum off and on),
flr_topk_abs_select (with the accumulate pass's level-1 histogram and with its
own), flr_sparsefed_apply, flr_topk_abs_mask, the whole
SparseFedDefense.aggregate_flat, and flr_rlr_fedavg on the same matrix — the
existing kernel with the same K*P*4 read, the yardstick of the accumulate pass.
Event-timed on one stream: every call warmed up, then REPS rounds that time the
calls in turn (N back-to-back calls per window), so drift over the run hits all
of them alike; the table gives each call's median window, its min-max spread,
the bytes the algorithm moves (computed from the shapes) and their rate as a
share of the HBM peak.
What each window works on.  The accumulate windows update memories of their own
in place: the work per call does not depend on their content.  The select, mask
and apply windows work on Ws, one accumulate's result from an empty memory, and
hs, the level-1 histogram that accumulate counted: nothing else writes either,
and before and after the timing the tool checks that the select with hs equals
the select with its own level-1 pass on Ws and that exactly k coordinates are
selected.  The apply zeroes what it applies, so its window restores its memory
from Ws before every call (a 2 * 4 * P byte copy, timed alone in the row above
it: the apply's own time is the difference); sel and the select's scratch are
recomputed from Ws, untimed, before each mask and apply window, because the
other windows' selects share that scratch.
Under a kernel tracer (rocprofv3 --kernel-trace --stats -- python
tools/sparsefed_bench.py, in a run of its own) set N=3 REPS=1.
Env: K, P, N (calls per window), REPS, KFRAC (k = ceil(KFRAC * P), the
defense's rule), RHO."""
import math, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-fl-security_amd"))
import torch
from flr import ops
from flr.defenses import get_defense
from flr.matrix import ClientMatrix
from flr.models.multimodal import ModelSpec, num_params
from flr.workload import update_matrix

HBM_TBS = 8.0  # the MI355X's peak HBM rate, TB/s
K = int(os.environ.get("K", 128))
P = int(os.environ.get("P", 0)) or num_params(ModelSpec())
N = int(os.environ.get("N", 30)); REPS = int(os.environ.get("REPS", 5))
KFRAC = float(os.environ.get("KFRAC", 0.05)); RHO = float(os.environ.get("RHO", 0.5))
assert torch.cuda.is_available(), "sparsefed_bench needs a GPU"
data = update_matrix(K, P, f=0, device="cuda")
X = data[:, :P]
cm = ClientMatrix(data, P, [torch.Size([P])])
n = torch.arange(1, K + 1, dtype=torch.int64, device="cuda")
g = ops.fedavg(X, torch.ones_like(n))  # the rows' mean
k = min(P, max(1, math.ceil(KFRAC * P)))
out = torch.empty(P, device="cuda"); out2 = torch.empty(P, device="cuda")
Wa = torch.zeros(P, device="cuda"); W2 = torch.zeros(P, device="cuda"); U2 = torch.zeros(P, device="cuda")
mask = torch.empty(P, dtype=torch.uint8, device="cuda")
norms = ops.row_norms(X, center=g)
beta, stats, _ = ops.sparsefed_weights(norms, diagnostics=True)
# the select's, mask's and apply's vector and its own level-1 histogram: written here, then only read
Ws = torch.zeros(P, device="cuda")
_, hs, _ = ops.sparsefed_accumulate_(X, g, beta, Ws, diagnostics=True)
Wt = torch.empty(P, device="cuda")   # the apply's memory, restored from Ws before every call
cur = {}
def fresh_sel():
    cur["sel"] = ops.topk_abs_select(Ws, k, hist=hs)
def check_select():
    """hs is Ws's histogram: both selects agree, and k coordinates are selected."""
    a, b = ops.topk_abs_select(Ws, k, hist=hs), ops.topk_abs_select(Ws, k)
    assert torch.equal(a, b), (a.tolist(), b.tolist())
    assert int(ops.topk_abs_mask(Ws, b).sum().item()) == k
    return [int(x) & 0xffffffff for x in b.tolist()]
sel_words = check_select()
def restore_and_apply():
    Wt.copy_(Ws)
    ops.sparsefed_apply_(g, Wt, cur["sel"], out=out, mask=True)
L, ngood, nclip = stats.cpu().tolist()
d0 = get_defense("sparsefed", {"k": KFRAC})
d1 = get_defense("sparsefed", {"k": KFRAC, "momentum": RHO})
kp, p4 = 4 * K * P, 4 * P
rows = int((beta != 0).sum().item())
calls = [  # name, call, bytes moved, untimed preparation of a window
    ("rlr_fedavg (yardstick)", lambda: ops.rlr_fedavg(X, n, g, 8, 1.0, out=out2, diagnostics=True), kp + 3 * p4, None),
    ("sparsefed_accumulate", lambda: ops.sparsefed_accumulate_(X, g, beta, Wa, diagnostics=True),
     4 * rows * P + 3 * p4, None),
    (f"sparsefed_accumulate rho={RHO:g}", lambda: ops.sparsefed_accumulate_(X, g, beta, W2, U2, RHO, diagnostics=True),
     4 * rows * P + 5 * p4, None),
    ("row_norms", lambda: ops.row_norms(X, center=g), kp + p4, None),
    ("sparsefed_weights", lambda: ops.sparsefed_weights(norms, diagnostics=True), 12 * K, None),
    ("topk_abs_select (hist given)", lambda: ops.topk_abs_select(Ws, k, hist=hs), 3 * p4, None),
    ("topk_abs_select (own level 1)", lambda: ops.topk_abs_select(Ws, k), 4 * p4, None),
    ("topk_abs_mask", lambda: ops.topk_abs_mask(Ws, cur["sel"], out=mask), p4 + P, fresh_sel),
    ("copy of W (the restore alone)", lambda: Wt.copy_(Ws), 2 * p4, None),
    ("copy of W, then sparsefed_apply + mask", restore_and_apply, 2 * p4 + 3 * p4 + P + 4 * k, fresh_sel),
    ("aggregate_flat", lambda: d0.aggregate_flat(cm, [], global_flat=g), kp + 4 * rows * P + 11 * p4 + P, None),
    (f"aggregate_flat rho={RHO:g}", lambda: d1.aggregate_flat(cm, [], global_flat=g),
     kp + 4 * rows * P + 15 * p4 + P, None),
]
def window(fn):
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(N): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / N
for _, fn, _, prep in calls:
    if prep: prep()
    for _ in range(3): fn()
torch.cuda.synchronize()
times = {name: [] for name, _, _, _ in calls}
for _ in range(REPS):
    for name, fn, _, prep in calls:
        if prep:
            prep(); torch.cuda.synchronize()
        times[name].append(window(fn))
assert check_select() == sel_words   # Ws and hs were only read
assert int(mask.sum().item()) == k
print(f"K={K} P={P} k={k}: K*P*4 = {kp / 1e9:.3f} GB, L = {L:.4g}, {int(nclip)} of {int(ngood)} rows clipped, "
      f"{rows} rows read, {N} calls per window, {REPS} windows per call; HBM peak {HBM_TBS:g} TB/s", flush=True)
print(f"the select on Ws: T = {sel_words[0]:#010x}, n_gt = {sel_words[1]}, r = {sel_words[2]}, flags = {sel_words[3]}; "
      f"the same with the accumulate pass's histogram and with its own, before and after the timing", flush=True)
print("| call | median ms | min | max | GB moved | TB/s | share of HBM peak |\n|---|---|---|---|---|---|---|")
med = {}
for name, _, nbytes, _ in calls:
    t = med[name] = statistics.median(times[name])
    rate = nbytes / t / 1e9
    print(f"| {name} | {t:.3f} | {min(times[name]):.3f} | {max(times[name]):.3f} | {nbytes / 1e9:.3f} | "
          f"{rate:.2f} | {100 * rate / HBM_TBS:.0f} % |", flush=True)
apply_ms = med["copy of W, then sparsefed_apply + mask"] - med["copy of W (the restore alone)"]
rest = med["aggregate_flat"] - med["row_norms"] - med["sparsefed_accumulate"]
print(f"sparsefed_apply + mask alone (the difference of the two rows): {apply_ms:.3f} ms; aggregate_flat minus "
      f"row_norms minus sparsefed_accumulate: {rest:.3f} ms", flush=True)
m = d0.get_metrics()
print(f"last aggregate_flat: k {m['k']}, threshold {m['threshold']:.4g}, clipped {m['clipped']}, "
      f"dropped {m['dropped']}", flush=True)
