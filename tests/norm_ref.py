"""Reference and fp32 yardstick for the channel LayerNorm kernels of csrc/norm.hip (plain torch / numpy on the CPU; nothing from sda_amd).

  stats64, bwd64          the operation in float64 on the fp32 inputs: what the kernels are compared with
  stats32_seq, bwd32_seq  the same formulas in float32, summed sequentially over channels (the arithmetic of ln_stats_kernel and
                          ln_bwd_kernel): they exist only to size the tolerance -- a kernel may be `FACTOR` times as far from float64
                          as this plain fp32 evaluation is ON THE SAME INPUTS, never less than `FLOOR_ULPS` ulps of the tensor's scale

x is planar (n, c, h, w); `mod` is the flat row of floats that starts at the pointer the kernel is given, and `mod_sn_kind` says how
the per-image rows lie in it: 'none' (no modulation), 'image' (rows of c), 'column' (rows of c + COLUMN_PAD: a column block of a wider
modulation matrix) or 'shared' (one row for every image, mod_sn = 0)."""
import numpy as np
import torch

COLUMN_PAD = 37          # a 'column' view has rows of c + COLUMN_PAD floats ...
COLUMN_START = 5         # ... and starts this many floats into its buffer (4-byte alignment only)
FACTOR = 4.0             # lane partials, shuffle trees, LDS partials, pairwise cell sums against one sequential sum
FLOOR_ULPS = 2.0
ULP32 = 2.0 ** -23


def mod_sn(kind: str, c: int) -> int:
    return {'none': 0, 'image': c, 'column': c + COLUMN_PAD, 'shared': 0}[kind]


def mod_rows(mod, kind: str, n: int, c: int):
    """(n, c) rows the kernel adds to image 0 .. n-1 (None without modulation)."""
    if kind == 'none':
        return None
    sn = mod_sn(kind, c)
    return torch.stack([mod[i * sn:i * sn + c] for i in range(n)])


def _u64(x, mod, kind):
    n, c = x.shape[:2]
    u = x.reshape(n, c, -1).double()
    rows = mod_rows(mod, kind, n, c)
    return u if rows is None else u + rows.double()[:, :, None]


def _cells64(gh, n, c, h, w, pool):
    return gh.double().reshape(n, c, h, pool[0], w, pool[1]).sum((-1, -3)).reshape(n, c, h * w)


def stats64(x, mod, mod_sn_kind, eps, unbiased):
    """(mean, rstd), float64, each (n * hw,)."""
    u = _u64(x, mod, mod_sn_kind)
    c = u.shape[1]
    mean = u.mean(1)
    var = ((u - mean[:, None]) ** 2).sum(1) / (c - 1 if unbiased else c)
    return mean.reshape(-1), (1.0 / torch.sqrt(var + eps)).reshape(-1)


def bwd64(gh, x, mod, mean, rstd, unbiased, pool, res, mod_sn_kind='image'):
    """gx = rstd * (g - mean_c(g) - h * sum_c(g h) / (c-1 | c)) + res in float64, with g the pool[0] x pool[1] cell sum of gh and
    h = (x + mod - mean) * rstd on the mean and rstd it is GIVEN (so a backward test does not depend on the statistics kernels)."""
    n, c, h, w = x.shape
    u = _u64(x, mod, mod_sn_kind)
    m, r = mean.double().reshape(n, 1, -1), rstd.double().reshape(n, 1, -1)
    hh = (u - m) * r
    g = _cells64(gh, n, c, h, w, pool)
    a = g.mean(1, keepdim=True)
    b = (g * hh).sum(1, keepdim=True) / (c - 1 if unbiased else c)
    out = r * (g - a - hh * b)
    if res is not None:
        out = out + res.double().reshape(n, c, -1)
    return out.reshape(n, c, h, w)


def _u32(x, mod, kind):
    n, c = x.shape[:2]
    u = x.reshape(n, c, -1).numpy().astype(np.float32)
    rows = mod_rows(mod, kind, n, c)
    return u if rows is None else u + rows.numpy().astype(np.float32)[:, :, None]


def stats32_seq(x, mod, mod_sn_kind, eps, unbiased):
    u = _u32(x, mod, mod_sn_kind)
    n, c, hw = u.shape
    s = np.zeros((n, hw), np.float32)
    for k in range(c):
        s += u[:, k]
    m = s / np.float32(c)
    q = np.zeros((n, hw), np.float32)
    for k in range(c):
        d = u[:, k] - m
        q += d * d
    var = q / np.float32(c - 1 if unbiased else c)
    rstd = np.float32(1.0) / np.sqrt(var + np.float32(eps))
    assert m.dtype == np.float32 and rstd.dtype == np.float32
    return torch.from_numpy(m.reshape(-1)), torch.from_numpy(rstd.reshape(-1))


def bwd32_seq(gh, x, mod, mean, rstd, unbiased, pool, res, mod_sn_kind='image'):
    n, c, h, w = x.shape
    u = _u32(x, mod, mod_sn_kind)
    m = mean.numpy().astype(np.float32).reshape(n, 1, -1)
    r = rstd.numpy().astype(np.float32).reshape(n, 1, -1)
    hh = (u - m) * r
    g6 = gh.numpy().astype(np.float32).reshape(n, c, h, pool[0], w, pool[1])
    g = g6[:, :, :, 0, :, 0].copy()
    if pool[1] == 2:
        g += g6[:, :, :, 0, :, 1]
    if pool[0] == 2:
        g += g6[:, :, :, 1, :, 0]
        if pool[1] == 2:
            g += g6[:, :, :, 1, :, 1]
    g = g.reshape(n, c, -1)
    s1 = np.zeros((n, h * w), np.float32)
    s2 = np.zeros((n, h * w), np.float32)
    for k in range(c):
        s1 += g[:, k]
        s2 += g[:, k] * hh[:, k]
    a = (s1 / np.float32(c))[:, None]
    b = (s2 / np.float32(c - 1 if unbiased else c))[:, None]
    out = r * (g - a - hh * b)
    if res is not None:
        out = out + res.numpy().astype(np.float32).reshape(n, c, -1)
    assert out.dtype == np.float32
    return torch.from_numpy(out.reshape(n, c, h, w))


def scale_err(got, ref) -> float:
    """max |got - ref| relative to max |ref| (0 / 0 = 0: an all-zero reference met exactly)."""
    d = float((got.double() - ref.double()).abs().max())
    s = float(ref.double().abs().max())
    return 0.0 if d == 0.0 else d / max(s, 1e-300)


def rel_err(got, ref) -> float:
    """largest elementwise relative error (the reference has no zero: rstd)."""
    return float(((got.double() - ref.double()) / ref.double()).abs().max())


def bound(yardstick_err: float) -> float:
    return max(FACTOR * yardstick_err, FLOOR_ULPS * ULP32)
