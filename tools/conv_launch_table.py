"""The tap-major GEMM engine's launch decisions as a table: for each knob
setting and each convolution geometry, what the host-only queries of the C API
answer (workspace, clip-norm slots, resident forms, fused data gradient, the
per-class split-K counts), and flr_bgemm_workspace for the batched-GEMM shapes
the native trainers size for.  No GPU: nothing is launched.
tests/golden/conv_launch_table.json is this table at the commit before the
launch policy moved into conv_t_launch.h; tests/test_conv_launch_host.py
recomputes it.
Printed packed (pack / unpack below).
usage: python tools/conv_launch_table.py > table.json"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multimodal-fl-security_amd"))
from flr import _capi

# (Cin, H, W, Cout, KH, KW, stride, pad): ResNet-18 at 32 x 32 inputs, then a Cout
# that is no multiple of 128, odd images (7 x 7, 3 x 3: the weight gradient's
# scalar-load plan) and a stride-4 shape (16 parity classes)
SHAPES = {
    "l1": (64, 8, 8, 64, 3, 3, 1, 1),
    "l2a": (64, 8, 8, 128, 3, 3, 2, 1),
    "l2ds": (64, 8, 8, 128, 1, 1, 2, 0),
    "l2b": (128, 4, 4, 128, 3, 3, 1, 1),
    "l3a": (128, 4, 4, 256, 3, 3, 2, 1),
    "l3b": (256, 2, 2, 256, 3, 3, 1, 1),
    "l4a": (256, 2, 2, 512, 3, 3, 2, 1),
    "l4ds": (256, 2, 2, 512, 1, 1, 2, 0),
    "l4b": (512, 1, 1, 512, 3, 3, 1, 1),
    "ragged": (64, 8, 8, 192, 3, 3, 1, 1),
    "hw7": (64, 7, 7, 128, 3, 3, 1, 1),
    "hw3": (128, 3, 3, 128, 3, 3, 1, 1),
    "s4": (64, 8, 8, 64, 5, 5, 4, 2),
}
CLIENTS = (1, 4, 16, 32, 128)
BATCHES = (8, 16, 32)

SETTINGS = ([("default", None, None)] +
            [(f"{n}={v}", n, v) for n, v in (
                ("FLR_CONV_FILL", "0"), ("FLR_CONV_NARROW", "0"), ("FLR_CONV_RESIDENT", "0"),
                ("FLR_WGRAD_RESIDENT", "0"), ("FLR_GEMM", "pipe"), ("FLR_GEMM", "f32"))] +
            [(f"FLR_CONV_TILE={t}", "FLR_CONV_TILE", str(t)) for t in (11, 12, 21, 22, 13, 31, 14, 41)] +
            [("FLR_DGRAD_FUSED=0", "FLR_DGRAD_FUSED", "0"), ("FLR_DGRAD_FUSED=1", "FLR_DGRAD_FUSED", "1"),
             ("FLR_BGEMM_TILE=11", "FLR_BGEMM_TILE", "11"), ("FLR_BGEMM_TILE=22", "FLR_BGEMM_TILE", "22")])


def bgemm_shapes(B):
    """(M, N, R) of every flr_bgemm the ResNet+GRU trainer (train_clients.hip) and
    the ViT-S + BERT-mini trainer (train_vit_bert.hip) size a workspace for."""
    out = []

    def linear(rows, n_out, n_in):  # forward, data gradient, weight gradient
        out.extend([(rows, n_out, n_in), (rows, n_in, n_out), (n_out, n_in, rows)])

    T, H, E, F, C, Dimg = 16, 256, 128, 256, 10, 512
    N = T * B
    linear(N, 3 * H, E)          # gi / W_ih
    linear(B, 3 * H, H)          # gh (unfused GRU)
    out.append((3 * H, H, T * B))  # dW_hh
    linear(B, F, Dimg)
    linear(B, F, H)              # fc1's two halves
    linear(B, C, F)              # fc2
    Dv, Mv, Tv, Db, Fb, Tb = 384, 1536, 65, 256, 1024, 16
    linear(B * 64, Dv, 48)       # patch embedding
    for rows, D, Fh in ((B * Tv, Dv, Mv), (B * Tb, Db, Fb)):
        linear(rows, 3 * D, D)   # qkv
        linear(rows, D, D)       # proj
        linear(rows, Fh, D)      # fc1
        linear(rows, D, Fh)      # fc2
    linear(B, Db, Db)            # pooler
    linear(B, F, Dv)
    linear(B, F, Db)             # fusion fc1's two halves
    return sorted(set(out))


def conv_row(lib, K, B, shape):
    Cin, H, W, Cout, KH, KW, stride, pad = shape
    geo = (K, B, Cin, H, W, Cout, KH, KW, stride, pad)
    ws = int(lib.flr_conv2d_t_workspace(*geo))
    row = [ws, int(lib.flr_conv2d_bwd_weight_t_sq_slots(*geo)), lib.flr_conv2d_wgrad_resident_ok(*geo),
           lib.flr_conv2d_resident_ok(*geo, 0), lib.flr_conv2d_resident_ok(*geo, 1),
           lib.flr_conv2d_dgrad_fused_supported(*geo), lib.flr_conv2d_dgrad_fused_preferred(*geo, 0),
           lib.flr_conv2d_dgrad_fused_preferred(*geo, 1)]
    for c in range(stride * stride):
        row.extend(lib.flr_conv2d_dgrad_class_splits(*geo, c, b) for b in (0, ws // 2, ws))
    return row


def table_for_current_knobs():
    lib = _capi.lib()
    conv = {f"{name}/K{K}/B{B}": conv_row(lib, K, B, shape)
            for name, shape in SHAPES.items() for K in CLIENTS for B in BATCHES}
    shapes = sorted({s for B in BATCHES for s in bgemm_shapes(B)})
    bgemm = {f"{M}x{N}x{R}/K{K}": int(lib.flr_bgemm_workspace(K, M, N, R)) for M, N, R in shapes for K in CLIENTS}
    return {"conv": conv, "bgemm": bgemm}


def table():
    """{setting: {"conv": {"shape/K/B": [workspace, sq_slots, wgrad_resident, resident fwd, resident dgrad,
    fused supported, fused preferred, fused preferred with shortcut, class 0 splits at workspace 0 / half /
    full, class 1 ...]}, "bgemm": {"MxNxR/K": workspace}}}; each knob is restored to the environment's value."""
    out = {}
    for label, name, value in SETTINGS:
        if name:
            _capi.set_knob(name, value)
        try:
            out[label] = table_for_current_knobs()
        finally:
            if name:
                _capi.set_knob(name, os.environ.get(name))
    return out


def pack(t):
    """The table without its repetition (a few hundred distinct conv rows fill its
    3705 entries, and no knob here moves a batched-GEMM workspace): the distinct rows
    once, per setting and shape the row numbers in (K, B) order, the default
    setting's batched-GEMM sizes in K order and, per setting, only the entries
    that differ from them.  unpack() gives the table back."""
    rows = sorted({tuple(r) for s in t.values() for r in s["conv"].values()})
    number = {r: i for i, r in enumerate(rows)}
    base = t["default"]["bgemm"]
    mnr = sorted({k.split("/")[0] for k in base}, key=lambda s: [int(v) for v in s.split("x")])
    return {
        "clients": list(CLIENTS), "batches": list(BATCHES), "rows": [list(r) for r in rows],
        "bgemm": {s: [base[f"{s}/K{K}"] for K in CLIENTS] for s in mnr},
        "settings": {label: {"conv": {name: [number[tuple(s["conv"][f"{name}/K{K}/B{B}"])]
                                             for K in CLIENTS for B in BATCHES] for name in SHAPES},
                             "bgemm": {k: v for k, v in s["bgemm"].items() if v != base[k]}}
                     for label, s in t.items()},
    }


def unpack(p):
    base = {f"{s}/K{K}": v for s, vals in p["bgemm"].items() for K, v in zip(p["clients"], vals)}
    kb = [(K, B) for K in p["clients"] for B in p["batches"]]
    return {label: {"conv": {f"{name}/K{K}/B{B}": p["rows"][i] for name, idx in s["conv"].items()
                             for (K, B), i in zip(kb, idx)},
                    "bgemm": {**base, **s["bgemm"]}}
            for label, s in p["settings"].items()}


if __name__ == "__main__":
    p = pack(table())
    assert unpack(p) == table()
    # one line per top-level entry and per setting
    head = [json.dumps(k) + ":" + json.dumps(p[k], separators=(",", ":")) for k in ("clients", "batches", "rows", "bgemm")]
    sets = [json.dumps(k) + ":" + json.dumps(v, separators=(",", ":")) for k, v in p["settings"].items()]
    print("{\n" + ",\n".join(head) + ',\n"settings":{\n' + ",\n".join(sets) + "\n}\n}")
