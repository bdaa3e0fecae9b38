"""Per-layer timing of the client-batched conv kernels at the C3 shapes
(K=128 clients, B=32): fwd / dgrad / wgrad, us and TFLOP/s (useful FLOPs of
the valid taps).  usage: conv_bench.py [--only NAME] [--reps N] [--resident] [--shortcut] [--variants "A=1,B=2;C=3"]
--shortcut: a row "dg+ds" for l2a / l3a / l4a, the data gradient with the block's 1x1 shortcut folded in
(flr_conv2d_bwd_data_t_sc: two per-class call sequences, or one launch under FLR_DGRAD_FUSED).
--resident: columns for FLR_CONV_RESIDENT=0 | 1 | 0 | 1 (the resident-B form of layer1's fwd / dgrad), then
for FLR_WGRAD_RESIDENT=0 | 1 | 0 | 1 (the resident form of layer1's weight gradient).
--variants: extra env settings timed in the same process, interleaved with the
default (one column each; the kernels read FLR_GEMM / FLR_XCD per launch)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-fl-security_amd"))
import torch
from flr import _capi
from flr.nn import _workspace, _workspace_t, _stream, tap_major_ok

K, B = int(os.environ.get("K", 128)), 32
LAYERS = [  # name, Cin, H, Cout, k, stride, pad
    ("stem", 3, 32, 64, 7, 2, 3),
    ("l1", 64, 8, 64, 3, 1, 1),
    ("l2a", 64, 8, 128, 3, 2, 1),
    ("l2b", 128, 4, 128, 3, 1, 1),
    ("l2ds", 64, 8, 128, 1, 2, 0),
    ("l3a", 128, 4, 256, 3, 2, 1),
    ("l3b", 256, 2, 256, 3, 1, 1),
    ("l3ds", 128, 4, 256, 1, 2, 0),
    ("l4a", 256, 2, 512, 3, 2, 1),
    ("l4b", 512, 1, 512, 3, 1, 1),
    ("l4ds", 256, 2, 512, 1, 2, 0),
]



def _set_knobs(env):
    """The library reads FLR_* switches once at load: variants go through flr_set_knob."""
    from flr import _capi
    for k, v in env.items():
        if k.startswith("FLR_"):
            _capi.set_knob(k, v)

def taps(H, k, s, p):
    Ho = (H + 2 * p - k) // s + 1
    v = [kh for kh in range(k) if any(0 <= o * s - p + kh < H for o in range(Ho))]
    return len(v) ** 2, Ho


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    dev = "cuda"
    variants = [{}]
    if "--variants" in sys.argv:
        for v in sys.argv[sys.argv.index("--variants") + 1].split(";"):
            variants.append(dict(kv.split("=") for kv in v.split(",") if kv))
    if "--resident" in sys.argv:  # the resident-B form off / on, twice, alternated per op (after the library default)
        variants += [{"FLR_CONV_RESIDENT": v} for v in ("0", "1", "0", "1")]
        # then the resident weight gradient off / on, twice: only the wgrad row changes kernel over these
        # four columns, the fwd and dgrad rows show the drift
        variants += [{"FLR_WGRAD_RESIDENT": v} for v in ("0", "1", "0", "1")]
    print("variants:", variants, flush=True)
    tot = [0.0] * len(variants)
    for name, Cin, H, Cout, k, s, p in LAYERS:
        if only and name != only:
            continue
        nt, Ho = taps(H, k, s, p)
        x = torch.randn(B, K * Cin, H, H, device=dev)
        w = torch.randn(K, Cout, Cin, k, k, device=dev) * 0.05
        y = torch.empty(B, K * Cout, Ho, Ho, device=dev)
        dy = torch.randn_like(y)
        dx = torch.empty_like(x)
        dw = torch.empty_like(w)
        geom = (K, B, Cin, H, H, Cout, k, k, s, p)
        tm = tap_major_ok(Cin, Cout) and "--generic" not in sys.argv
        sfx = "_t" if tm else ""
        ws, n = (_workspace_t if tm else _workspace)(geom, dev)
        wsp = None if ws is None else ws.data_ptr()
        st = _stream(x)
        calls = {
            "fwd": lambda: _capi.call("flr_conv2d_fwd" + sfx, x.data_ptr(), w.data_ptr(), y.data_ptr(), *geom, wsp,
                                      n, st),
            "dgrad": lambda: _capi.call("flr_conv2d_bwd_data" + sfx, dy.data_ptr(), w.data_ptr(), dx.data_ptr(),
                                        *geom, wsp, n, st),
            "wgrad": lambda: _capi.call("flr_conv2d_bwd_weight" + sfx, x.data_ptr(), dy.data_ptr(), dw.data_ptr(),
                                        *geom, *((0,) if tm else ()), wsp, n, st),  # dead taps skipped, as in training
        }
        if "--shortcut" in sys.argv and tm and s == 2 and k == 3:
            dyd = torch.randn_like(y)
            wd = torch.randn(K, Cout, Cin, 1, 1, device=dev) * 0.05
            wst = k * k * Cin * Cout  # (k is rebound by the variant loop below)
            calls["dg+ds"] = lambda: _capi.call("flr_conv2d_bwd_data_t_sc", dy.data_ptr(), w.data_ptr(),
                                                wst, None, dx.data_ptr(), *geom, dyd.data_ptr(),
                                                wd.data_ptr(), Cin * Cout, Cout, wsp, n, st)
        flops = 2.0 * K * B * Ho * Ho * Cout * Cin * nt
        for op, fn in calls.items():
            if name == "stem" and op == "dgrad":
                continue
            cols = []
            for vi, env in enumerate(variants):
                saved = {k: os.environ.get(k) for k in env}
                os.environ.update(env)
                _set_knobs(env)
                fn()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                for k, v in saved.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
                _set_knobs(saved)
                us = e0.elapsed_time(e1) * 1e3 / reps
                tot[vi] += us
                cols.append(f"{us:9.1f} us {flops / us / 1e6:7.1f} TF/s")
            print(f"{name:5s} {op:6s} " + " | ".join(cols), flush=True)
    print("sum " + " | ".join(f"{t / 1e3:.2f} ms" for t in tot) + " (one of each per layer)")


if __name__ == "__main__":
    main()
