"""Reference model of the fused clip + SGD-momentum step in numpy, the contract
of flr_clip_sgd_step and flr_clip_sgd_step_blocked* / _phase (include/flr.h).
A helper module, not a test file.  The library builds with -ffp-contract=off
and the kernels write every rounding out, so ``step`` is their result bit for
bit: one rounding for g*coef, an FMA for the weight decay, two roundings for
buf.mul_(mom).add_(g), an FMA for the parameter update."""
import numpy as np

F32 = np.float32


def fma32(a, b, c):
    """The correctly rounded fp32 a*b + c, elementwise (no math.fma before
    Python 3.13): the exact product in fp64, the sum rounded to odd (TwoSum's
    error says which way the exact sum lies), then one rounding to fp32.
    Round-to-odd keeps a sticky bit 29 places below fp32's last one, so the
    second rounding cannot land on a false tie."""
    a = np.asarray(a, F32).astype(np.float64)
    b = np.asarray(b, F32).astype(np.float64)
    c = np.asarray(c, F32).astype(np.float64)
    a, b, c = np.broadcast_arrays(a, b, c)
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b                       # 24 x 24 bits: exact
        s = p + c
        t = s - p
        e = (p - (s - t)) + (c - t)     # TwoSum: p + c = s + e exactly
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (e != 0) & even
        toward = np.where(e > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(F32)


def clip_coef(norm, max_norm, dtype=F32):
    """clip_grad_norm_'s coefficient min(1, max_norm / (norm + 1e-6)), every
    operand and rounding in ``dtype`` (the kernels: fp32)."""
    norm = np.asarray(norm, dtype)
    with np.errstate(divide="ignore"):
        c = (dtype(max_norm) / (norm + dtype(1e-6))).astype(dtype)
    return np.where(c < dtype(1), c, dtype(1)).astype(dtype)


def step(x, g, m, coef, lr, mom, wd, first):
    """One optimizer step in fp32: (x', m').  coef broadcasts against g (one
    value per client row); m is not read on a first step."""
    x = np.asarray(x, F32)
    g = np.asarray(g, F32)
    lr, mom, wd = F32(lr), F32(mom), F32(wd)
    gp = (g * np.asarray(coef, F32)).astype(F32)
    if wd != 0:
        gp = fma32(wd, x, gp)
    if first:
        buf = gp
    else:
        buf = ((np.asarray(m, F32) * mom).astype(F32) + gp).astype(F32)
    return fma32(-lr, buf, x), buf


def step64(x, g, m, coef, lr, mom, wd, first):
    """The same formula in float64 with no fp32 rounding: ties ``step`` to
    torch.optim.SGD + clip_grad_norm_ (tests/test_sgd_ref_host.py)."""
    x = np.asarray(x, np.float64)
    gp = np.asarray(g, np.float64) * coef
    if wd != 0:
        gp = gp + wd * x
    buf = gp if first else np.asarray(m, np.float64) * mom + gp
    return x - lr * buf, buf

# flr_clip_sgd_step_phase: at most MAX_BLOCKS parameter blocks a call, run as
# launches of at most BLOCKS_PER_LAUNCH (include/flr.h; MAXB * MAX_PARTS in
# csrc/train_step.hip)
BLOCKS_PER_LAUNCH = 80
MAX_BLOCKS = 640
