"""Time the fused GRU step kernels (flr_gru_fwd_fused / flr_gru_bwd_fused) at
the C3 text-branch shape under each (waves, k-steps-per-group) variant.
usage: gru_bench.py [K B T H]
       gru_bench.py --seq [B T H [K,K,...]]
                                    the per-step launches (T forward; 1 + (T - 1) backward) against the
                                    one-launch flr_gru_fwd_seq / flr_gru_bwd_seq, alternated off / on / off / on
                                    in one process at K = 128, 32 and 16 (C3, C2, the 8-GPU share)"""
import ctypes, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multimodal-fl-security_amd"))
import torch
from flr import _capi


def seq_ab(K, B, T, H, n=20):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=dev, generator=g) * 0.1
    from flr.nn import _gru_packed
    gi, bhh = r(K, B, T, 3 * H), r(K, 3 * H)
    hseq, gates = r(K, T + 1, B, H), torch.sigmoid(r(K, T, B, 4 * H))
    whhP, whhT = r(K, _gru_packed(3, H, H)), r(K, _gru_packed(1, H, 3 * H))
    dh, dgh, dgi, dd = r(K, B, H), r(K, T, B, 3 * H), r(K, B, T, 3 * H), r(K, B, H)
    lib = _capi.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda x: ctypes.c_void_p(x.data_ptr())

    def fwd_steps():
        rc = 0
        for t in range(T):
            rc |= lib.flr_gru_fwd_fused_ex(P(gi), P(whhP), 0, P(bhh), P(hseq), P(gates), K, B, T, H, t, st)
        return rc

    def bwd_steps():
        rc = lib.flr_gru_bwd_step(P(dh), P(gates), P(hseq), P(dgh), P(dgi), P(dd), K, B, T, H, T - 1, st)
        for t in range(T - 1, 0, -1):
            rc |= lib.flr_gru_bwd_fused_ex(P(whhT), 0, P(gates), P(hseq), P(dgh), P(dgi), P(dd), None, K, B, T, H, t, st)
        return rc

    fwd_seq = lambda: lib.flr_gru_fwd_seq(P(gi), P(whhP), 0, P(bhh), P(hseq), P(gates), K, B, T, H, st)
    bwd_seq = lambda: lib.flr_gru_bwd_seq(P(whhT), 0, P(gates), P(hseq), P(dh), P(dgh), P(dgi), P(dd), None,
                                          K, B, T, H, st)

    def timeit(fn):
        for _ in range(3):
            assert fn() == 0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n * 1e3

    wmb = 4 * K * 3 * H * H / 1e6
    for name, steps, seq, nst in [("fwd", fwd_steps, fwd_seq, T), ("bwd", bwd_steps, bwd_seq, max(T - 1, 1))]:
        us = [timeit(f) for f in (steps, seq, steps, seq)]
        per = [u / nst for u in us]
        print(f"K={K:4d} {name}  pass us: per-step {us[0]:8.1f} {us[2]:8.1f} | seq {us[1]:8.1f} {us[3]:8.1f}"
              f"  ||  us per time step: per-step {per[0]:6.2f} {per[2]:6.2f} | seq {per[1]:6.2f} {per[3]:6.2f}"
              f"  ||  seq W_hh stream {wmb / min(per[1], per[3]):5.2f} TB/s", flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--seq":
        B, T, H = (int(a) for a in sys.argv[2:5]) if len(sys.argv) > 4 else (32, 16, 256)
        Ks = [int(k) for k in sys.argv[5].split(",")] if len(sys.argv) > 5 else (128, 32, 16)
        for K in Ks:
            seq_ab(K, B, T, H)
        return
    K, B, T, H = (int(a) for a in sys.argv[1:5]) if len(sys.argv) > 4 else (128, 32, 16, 256)
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=dev, generator=g) * 0.1
    gi, whh, bhh = r(K, B, T, 3 * H), r(K, 3 * H, H), r(K, 3 * H)
    hseq, gates = r(K, T + 1, B, H), r(K, T, B, 4 * H)
    from flr.nn import _gru_packed
    whhP, whhT = r(K, _gru_packed(3, H, H)), r(K, _gru_packed(1, H, 3 * H))
    dgh, dgi, dd = r(K, T, B, 3 * H), r(K, B, T, 3 * H), r(K, B, H)
    dd0 = dd.clone()
    lib = _capi.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda x: ctypes.c_void_p(x.data_ptr())
    fwd = lambda: lib.flr_gru_fwd_fused(P(gi), P(whhP), P(bhh), P(hseq), P(gates), K, B, T, H, 5, st)
    bwd = lambda: lib.flr_gru_bwd_fused(P(whhT), P(gates), P(hseq), P(dgh), P(dgi), P(dd), None, K, B, T, H, 6, st)
    wbytes = 4 * K * 3 * H * H
    pack = lambda: lib.flr_gru_pack(P(whh), K, 3, H, H, 0, P(whhP), st)
    packT = lambda: lib.flr_gru_pack(P(whh), K, 1, H, 3 * H, 1, P(whhT), st)

    def timeit(fn, n=50):
        for _ in range(5):
            assert fn() == 0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n * 1e3

    for name, fn in [("pack W_hh", pack), ("pack W_hh^T", packT)]:
        us = timeit(fn)
        print(f"{name:12s} {us:8.2f} us  {2 * wbytes / us / 1e6:6.2f} TB/s (read + write)", flush=True)
    outs = {"fwd": lambda: (hseq[:, 6].clone(), gates[:, 5].clone()),
            "bwd": lambda: (dgh[:, 5].clone(), dgi[:, :, 5].clone(), dd.clone())}
    for var, env, fn in [("fwd", "FLR_GRU_FW", fwd), ("bwd", "FLR_GRU_BW", bwd)]:
        cfgs = ["8,2", "8,2s", "4,4", "2,8"] if var == "fwd" else ["8,2", "8,2s", "8,6", "4,12", "16,3"]
        ref = None
        for c in cfgs:
            os.environ[env] = c
            if var == "bwd":
                dd.copy_(dd0)  # the bwd step rewrites dh_direct in place: same input for every variant
            assert fn() == 0
            torch.cuda.synchronize()
            o = outs[var]()
            same = "" if ref is None else ("  bit-identical" if all(torch.equal(a, b) for a, b in zip(o, ref))
                                            else "  DIFFERS")
            ref = ref if ref is not None else o
            us = timeit(fn)
            print(f"{var} NW,G={c:5s} {us:8.2f} us  W_hh stream {wbytes / us / 1e6:6.2f} TB/s{same}", flush=True)
        os.environ.pop(env)


if __name__ == "__main__":
    main()
