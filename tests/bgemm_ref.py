"""CPU references for the batched-GEMM and row-sum tests (no GPU import).

int_operands: operands on which every correct form of flr_bgemm must return the
same exact integers, so the comparison needs no tolerance.  sum_rows_emulated:
the fp32 summation order that include/flr.h promises for flr_sum_rows[_ex].
splits / tile / grid: the documented launch policy restated, used only to
assert that a test shape reaches the path its id names."""
import functools

import numpy as np
import torch

BM = BN = 64        # the workgroup sub-tile (conv_common.h)
BK = 32             # reduction depth of one K-tile
MIN_KT = 32         # FLR_BGEMM_MINKT default: fewest K-tiles a split keeps
SR_CHUNK = 256      # flr_sum_rows_ex: rows per chunk
SR_MAXCHUNK = 64    # ... and the most chunks it takes before falling back to one pass


def cdiv(a, b):
    return -(-a // b)


def splits(M, N, R, sub):
    """Split-K count of one client's [M, N] product over R (choose_splits): doubled
    while below 16, the client has fewer than 16 workgroup tiles (64 x 64 tiles
    over sub sub-tiles each) and every split keeps at least MIN_KT K-tiles."""
    tiles = cdiv(M, BM) * cdiv(N, BN) // sub
    ktiles = cdiv(R, BK)
    S = 1
    while S < 16 and tiles * S < 16 and ktiles // (2 * S) >= MIN_KT:
        S *= 2
    return S


def tile(M, N, R):
    """Workgroup tile code (bgemm_tile): 22 = 128 x 128, 11 = 64 x 64."""
    return 22 if M >= 128 and N >= 128 and (R >= 256 or M * N >= 128 * 512) else 11


def plan(M, N, R, forced_tile=None):
    """(tile, S) the library chooses for one client's product."""
    t = forced_tile or tile(M, N, R)
    return t, splits(M, N, R, 4 if t == 22 else 1)


def grid(K, M, N, R, forced_tile=None):
    """Workgroups of the GEMM launch (launch_tiles)."""
    t, S = plan(M, N, R, forced_tile)
    e = 128 if t == 22 else 64
    return cdiv(N, e) * cdiv(M, e) * K * S


def operand_mode(t):
    """Load mode of the operand view t [K, rows, R] (bgemm_mode): "RK" (16-byte
    loads along r), "KR" (along the rows) or "G" (scalar gathers)."""
    s_k, s_row, s_r = t.stride()
    rows, R = t.shape[1], t.shape[2]
    al = t.data_ptr() % 16 == 0 and s_k % 4 == 0
    if s_r == 1 and al and s_row % 4 == 0 and R % 4 == 0:
        return "RK"
    if s_row == 1 and al and s_r % 4 == 0 and rows % 4 == 0:
        return "KR"
    return "G"


def workspace_bytes(K, M, N, R):
    S = max(splits(M, N, R, 1), splits(M, N, R, 4))
    return S * K * M * N * 4 if S > 1 else 0


@functools.lru_cache(maxsize=None)
def int_operands(K, M, N, R, seed=0):
    """Small integers stored in fp32: A [K, M, R], B [K, N, R] in [-3, 3], bias
    [K, N], add and aux [K, M, N] in [-8, 8], mask [K, M, N] in {0, 2}, and
    ref = the int64 bmm A B^T [K, M, N].

    Each value is its own bf16 hi term (mid = lo = 0), every product is an
    integer of magnitude <= 9 and every partial sum, with bias and addend, stays
    below 2^24: fp32 holds all of them exactly.  So the three-term kernel, the
    f32 form, either tile, any split count and any summation order must return
    exactly ref (+ bias + add).  Cached: callers must not modify the tensors."""
    assert 3 * 3 * R + 8 + 8 < 2 ** 24
    g = torch.Generator().manual_seed(seed * 7919 + K * 1000003 + M * 10007 + N * 101 + R)
    A = torch.randint(-3, 4, (K, M, R), generator=g)
    B = torch.randint(-3, 4, (K, N, R), generator=g)
    o = {"A": A.float(), "B": B.float(),
         "bias": torch.randint(-8, 9, (K, N), generator=g).float(),
         "add": torch.randint(-8, 9, (K, M, N), generator=g).float(),
         "aux": torch.randint(-8, 9, (K, M, N), generator=g).float(),
         "mask": torch.randint(0, 2, (K, M, N), generator=g).float() * 2.0,
         "ref": torch.bmm(A, B.transpose(1, 2))}
    assert o["ref"].dtype == torch.int64 and int(o["ref"].abs().max()) < 2 ** 24
    for v in ("A", "B", "bias", "add", "aux", "mask"):  # each value is a bf16
        assert torch.equal(o[v].bfloat16().float(), o[v])
    return o


def int_epilogue(o, bias=False, add=False, act="none", mask=False):
    """(pre, out) of flr_bgemm_ex on int_operands o, in int64: v = ref (+ bias)
    (+ add); pre = v; relu: max(v, 0) / drelu: v where aux > 0; (* mask)."""
    v = o["ref"].clone()
    if bias:
        v = v + o["bias"].long().unsqueeze(1)
    if add:
        v = v + o["add"].long()
    pre = v
    if act == "relu":
        v = v.clamp(min=0)
    elif act == "drelu":
        v = torch.where(o["aux"] > 0, v, torch.zeros_like(v))
    else:
        assert act == "none"
    if mask:
        v = v * o["mask"].long()
    return pre, v


def _eight(X):
    """[K, M, N] fp32 numpy -> [K, N]: accumulator j takes rows 8 i + j in order, the
    M % 8 tail rows go to accumulators 0.. in order, then the fixed tree."""
    K, M, N = X.shape
    a = np.zeros((8, K, N), np.float32)
    full = M // 8 * 8
    for i in range(0, full, 8):
        a += X[:, i:i + 8].transpose(1, 0, 2)  # a[j] += row 8 i + j: one rounded fp32 add each
    for j, m in enumerate(range(full, M)):
        a[j] += X[:, m]
    return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))


def sum_rows_emulated(X, chunked):
    """The fp32 order of flr_sum_rows (chunked=False) and of flr_sum_rows_ex with
    its workspace (chunked=True) on X [K, M, N]: the eight-accumulator sum over all
    rows; or, with 256 < M <= 64 * 256, that sum per 256-row chunk and the chunk
    partials added in chunk order starting from chunk 0's."""
    x = np.ascontiguousarray(X.detach().cpu().numpy(), dtype=np.float32)
    M = x.shape[1]
    if chunked and SR_CHUNK < M <= SR_MAXCHUNK * SR_CHUNK:
        s = _eight(x[:, :SR_CHUNK])
        for c in range(SR_CHUNK, M, SR_CHUNK):
            s = s + _eight(x[:, c:c + SR_CHUNK])
    else:
        s = _eight(x)
    assert s.dtype == np.float32
    return torch.from_numpy(s)


def sum_rows_workspace_bytes(K, M, N):
    if K < 1 or M <= SR_CHUNK or N < 1:
        return 0
    return cdiv(K * min(cdiv(M, SR_CHUNK), SR_MAXCHUNK) * N * 4, 256) * 256
