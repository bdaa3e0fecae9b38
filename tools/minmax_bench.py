"""Timing of the Min-Max / Min-Sum attacks (flr_minmax_rows) at C3's aggregate
shape (K=128, f=12 attackers, P = the default model's parameter count), next to
the passes it is made of on the same matrix in the same process:
flr_collude_rows (the mean/deviation pass: nb*P*4 bytes read), flr_pairwise_l2
on the benign rows (the Gram engine) and flr_row_norms around a center (the
yardstick of the statistics pass: the same fp32 difference and fp64 sum per
element, one sum per row where the statistics kernel keeps two).  One call reads
3 * nb * P * 4 bytes and writes nmal * P * 4.
Event-timed on one stream: every kernel warmed up, then REPS rounds that time
the kernels in turn (N back-to-back calls per window), so drift over the run
hits all of them alike; the table gives each kernel's median window and its
min-max spread.  Under `rocprofv3 --kernel-trace --stats` (a run of its own,
N=3 REPS=1) the per-kernel times of one call come from the trace: the
statistics pass is minmax::stats_kernel.
Env: K, F, P, N (calls per window), REPS."""
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-fl-security_amd"))
import torch
from flr import ops
from flr.models.multimodal import ModelSpec, num_params
from flr.workload import update_matrix

K = int(os.environ.get("K", 128)); F = int(os.environ.get("F", 12))
P = int(os.environ.get("P", 0)) or num_params(ModelSpec())
N = int(os.environ.get("N", 20)); REPS = int(os.environ.get("REPS", 5))
assert torch.cuda.is_available(), "minmax_bench needs a GPU"
X = update_matrix(K, P, f=0, device="cuda")[:, :P]
nb = K - F
g = ops.fedavg(X, [1] * K)
g.add_(0.01 * torch.randn(P, device="cuda"))
mean_out, std_out = torch.empty(P, device="cuda"), torch.empty(P, device="cuda")
gb = 4 * nb * P / 1e9      # one pass over the benign rows
wr = 4 * F * P / 1e9       # the attackers' rows written
kernels = [
    ("collude_rows ALIE (mean/std + write)", gb + wr, lambda: ops.collude_rows(X, F, ops.COLLUDE_ALIE, 0.5, mean_out, std_out)),
    ("pairwise_l2 gram (benign rows)", gb, lambda: ops.pairwise_l2(X[F:])),
    ("row_norms (center, benign rows)", gb, lambda: ops.row_norms(X[F:], g)),
    ("minmax_rows max std", 3 * gb + wr, lambda: ops.minmax_rows(X, F, ops.MINMAX_MAX, ops.PERTURB_STD)),
    ("minmax_rows sum sign", 3 * gb + wr, lambda: ops.minmax_rows(X, F, ops.MINMAX_SUM, ops.PERTURB_SIGN, g)),
    ("minmax_rows max unit", 3 * gb + wr, lambda: ops.minmax_rows(X, F, ops.MINMAX_MAX, ops.PERTURB_UNIT, g)),
]
def window(fn):
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(N): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / N
for _, _, fn in kernels:
    for _ in range(2): fn()
torch.cuda.synchronize()
times = {name: [] for name, _, _ in kernels}
for _ in range(REPS):
    for name, _, fn in kernels:
        times[name].append(window(fn))
print(f"K={K} f={F} P={P}: {gb:.3f} GB per pass over the {nb} benign rows, {wr:.3f} GB of attackers' rows, "
      f"{N} calls per window, {REPS} windows per kernel", flush=True)
gamma = ops.minmax_rows(X, F, ops.MINMAX_MAX, ops.PERTURB_STD).item()
print(f"gamma (max, std) = {gamma:.6g}", flush=True)
for name, nbytes, _ in kernels:
    t = statistics.median(times[name])
    print(f"{name:40s} {t:8.3f} ms  (min {min(times[name]):.3f}, max {max(times[name]):.3f})  "
          f"{nbytes:7.3f} GB  {nbytes / t * 1e3:8.1f} GB/s", flush=True)
