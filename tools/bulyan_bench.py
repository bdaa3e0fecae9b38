"""Timing of Bulyan's two kernels at C3's aggregate shape (K=128, f=25:
theta=78, beta=28, P=11.8 M), event-timed on one stream:
  ops.krum_select_iter next to ops.krum_select on the same D;
  ops.median_window_mean over the theta picks next to ops.trimmed_mean over
  the same rows (the yardstick: the same 4*theta*P bytes and the same sort).
Env: K, F, P, N (timed repeats)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-fl-security_amd"))
import torch
from flr import ops
from flr.workload import update_matrix

K = int(os.environ.get("K", 128)); f = int(os.environ.get("F", 25)); P = int(os.environ.get("P", 11_800_394))
N = int(os.environ.get("N", 10))
theta, beta = K - 2 * f, K - 4 * f
X = update_matrix(K, P, f=f, device="cuda")[:, :P]
torch.cuda.synchronize()
def timeit(fn, n=N):
    fn(); torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / n
print(f"K={K} f={f} theta={theta} beta={beta} P={P}", flush=True)
D = ops.pairwise_l2(X, "gram")
t_sel = timeit(lambda: ops.krum_select(D, f))
t_it = timeit(lambda: ops.krum_select_iter(D, f, theta))
print(f"krum_select        {t_sel:8.3f} ms", flush=True)
print(f"krum_select_iter   {t_it:8.3f} ms  ({theta + 1} launches)", flush=True)
rows = ops.krum_select_iter(D, f, theta)[1][:theta].contiguous()
t = (theta - beta) // 2
gb = 4 * theta * P / 1e9
t_tm = timeit(lambda: ops.trimmed_mean(X, t, rows=rows))
t_wm = timeit(lambda: ops.median_window_mean(X, beta, rows=rows))
t_md = timeit(lambda: ops.median_lower(X, rows=rows))
print(f"trimmed_mean rows  {t_tm:8.3f} ms  {gb / t_tm * 1e3:8.1f} GB/s  (t={t})", flush=True)
print(f"median_lower rows  {t_md:8.3f} ms  {gb / t_md * 1e3:8.1f} GB/s", flush=True)
print(f"window_mean rows   {t_wm:8.3f} ms  {gb / t_wm * 1e3:8.1f} GB/s  ratio to trimmed_mean {t_wm / t_tm:.3f}",
      flush=True)
