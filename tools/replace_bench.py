"""Timing of model replacement (flr_replace_strength + flr_scale_rows_from, with
the norms or the Gram matrix their mode needs) at C3's aggregate shape (K=128,
f=25 attackers, P = the default model's parameter count), next to
flr_collude_rows on the same matrix in the same process: the existing sibling
pass of that slot (it reads the nb benign rows and writes the f attackers' rows).
The scale's bytes-moved formula (include/flr.h) is 2 * f * P * 4 + P * 4; its
floor is that over the HBM rate (8 TB/s peak, about 6.3 TB/s achievable).
Event-timed on one stream, one pair of events per call: the attackers' rows are
restored from a copy between calls (outside the events), so every call scales
the same data by the same strengths.  Every kernel is warmed up, then REPS
rounds time the kernels in turn (N calls each), so drift over the run hits all of
them alike; the table gives each kernel's median call and its min-max spread.
Env: K, F, P, N (calls per round), REPS."""
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-fl-security_amd"))
import torch
from flr import ops
from flr.attacks import model_replacement_
from flr.models.multimodal import ModelSpec, num_params
from flr.workload import update_matrix

K = int(os.environ.get("K", 128)); F = int(os.environ.get("F", 25))
P = int(os.environ.get("P", 0)) or num_params(ModelSpec())
N = int(os.environ.get("N", 10)); REPS = int(os.environ.get("REPS", 5))
HBM_PEAK, HBM_ACHIEVABLE = 8.0e3, 6.3e3   # GB/s
assert torch.cuda.is_available(), "replace_bench needs a GPU"
X = update_matrix(K, P, f=0, device="cuda")[:, :P]
nb = K - F
g = ops.fedavg(X, [1] * K)
g.add_(0.01 * torch.randn(P, device="cuda"))
X0 = X[:F].clone()
gamma32 = torch.full((F,), K / F, device="cuda")
mean_out, std_out = torch.empty(P, device="cuda"), torch.empty(P, device="cuda")
row = 4 * P / 1e9
scale_gb = (2 * F + 1) * row            # the scale's formula
kernels = [
    ("collude_rows ALIE (sibling pass)", (nb + F) * row, lambda: ops.collude_rows(X, F, ops.COLLUDE_ALIE, 0.5, mean_out, std_out)),
    ("scale_rows_from (gamma = K / f)", scale_gb, lambda: ops.scale_rows_from(X, g, gamma32)),
    ("row_norms (center, all rows)", K * row, lambda: ops.row_norms(X, g)),
    ("rows_gram (center, all rows)", K * row, lambda: ops.rows_gram(X, g)),
    ("model_replacement none", scale_gb, lambda: model_replacement_(X, F, g)),
    ("model_replacement norm median", scale_gb + K * row, lambda: model_replacement_(X, F, g, stealth="norm")),
    ("model_replacement distance", scale_gb + K * row, lambda: model_replacement_(X, F, g, stealth="distance")),
]
def call(fn):
    X[:F].copy_(X0)
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record(); fn(); e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)
for _, _, fn in kernels:
    for _ in range(2): call(fn)
times = {name: [] for name, _, _ in kernels}
for _ in range(REPS):
    for name, _, fn in kernels:
        times[name] += [call(fn) for _ in range(N)]
print(f"K={K} f={F} P={P}: {row:.4f} GB per row, the scale's formula {scale_gb:.3f} GB "
      f"(floor {scale_gb / HBM_PEAK * 1e3:.3f} ms at 8 TB/s, {scale_gb / HBM_ACHIEVABLE * 1e3:.3f} ms at 6.3 TB/s), "
      f"{N * REPS} calls per kernel", flush=True)
X[:F].copy_(X0)
for stealth in ("none", "norm", "distance"):
    gam, status, flags = model_replacement_(X, F, g, stealth=stealth)
    print(f"stealth {stealth}: gamma {gam.min().item():.6g} .. {gam.max().item():.6g}, status counts "
          f"{torch.bincount(status, minlength=4).tolist()}, flags {flags.item()}", flush=True)
    X[:F].copy_(X0)
sib = statistics.median(times[kernels[0][0]])
for name, nbytes, _ in kernels:
    t = statistics.median(times[name])
    print(f"{name:34s} {t:8.3f} ms  (min {min(times[name]):.3f}, max {max(times[name]):.3f})  {nbytes:7.3f} GB  "
          f"{nbytes / t * 1e3:8.1f} GB/s  {100 * nbytes / t * 1e3 / HBM_PEAK:5.1f} % of 8 TB/s  "
          f"{t / sib:6.3f} x sibling", flush=True)
