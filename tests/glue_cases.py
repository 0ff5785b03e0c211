"""The shapes and seeded fp32 inputs that tests/test_glue_host.py (CPU: the references against the oracle) and tests/test_gpu_glue.py (the
kernels against the references) share, so that every reference is verified at the very shapes it then judges.  CPU tensors only."""
import math

import torch

# ---- sda_linear: every NT boundary of the column tile (32 / 64 / 96 / 128) and the second column block; both sides of the 16-deep K
# stage; one row, both sides of the 128-row tile, three row tiles
LIN_OUT = (1, 32, 33, 64, 65, 96, 97, 128, 129)
LIN_IN = (1, 15, 16, 17, 100)
LIN_ROWS = (1, 127, 128, 129, 300)
ACTS = (1, 2, 3, 4, 5)


def lin_full(out_f):
    return [(r, i, out_f) for r in LIN_ROWS for i in LIN_IN]


def lin_thin():
    """a Latin square through the cross product: 45 shapes, every out_f with every rows value and every in_f value once"""
    return [(LIN_ROWS[ri], LIN_IN[ki], LIN_OUT[oi]) for oi in range(len(LIN_OUT)) for ri in range(5) for ki in range(5)
            if (ri + ki + oi) % 5 == 0]


_master = {}


def _masters():
    if not _master:
        g = torch.Generator().manual_seed(20240611)
        _master.update(x=torch.randn(300, 129, generator=g), w=torch.randn(129, 129, generator=g), b=torch.randn(129, generator=g) * 0.5,
                       z=torch.randn(300, 129, generator=g) * 1.5, res=torch.randn(300, 129, generator=g))
    return _master


def lin_inputs(rows, in_f, out_f):
    """x [rows][in], w [out][in] at half of 1 / sqrt(in), b [out], z and res [rows][out] (pre-activations stay well inside the measured
    ranges of the activations)"""
    m = _masters()
    return dict(x=m['x'][:rows, :in_f].contiguous(), w=(m['w'][:out_f, :in_f] * (0.5 / math.sqrt(in_f))).contiguous(), b=m['b'][:out_f].contiguous(),
                z=m['z'][:rows, :out_f].contiguous(), res=m['res'][:rows, :out_f].contiguous())


# ---- sda_row_ln / sda_row_ln_bwd: one lane, two lanes, both sides of one wavefront, two registers per lane, a ragged and the full last
# register; rows on both sides of the 4-row workgroup
LN_F = (1, 2, 63, 64, 65, 128, 1000, 1024)
LN_ROWS = (1, 3, 4, 5, 130)
LN_EPS = 1e-5
# the row whose mean dwarfs its spread, 1e4 + N(0, 1): at 64 features the order-independent bound of the mean, 66 u 1e4 = 0.04, still leaves
# the bound of the variance well below the variance (at 1000 features it does not: the bound is void there, so the case is not run there)
LN_OFFSET = (5, 64)


def ln_cases():
    return [(rows, f, unbiased) for f in LN_F for rows in LN_ROWS for unbiased in (False, True) if not (unbiased and f == 1)]


def ln_inputs(rows, f, offset=False):
    g = torch.Generator().manual_seed(7000 + 13 * rows + f + (1 if offset else 0))
    x = torch.randn(rows, f, generator=g)
    x = x + 1e4 if offset else x * 2 + 0.7
    return dict(x=x, g=torch.randn(rows, f, generator=g), res=torch.randn(rows, f, generator=g))


# ---- fold family: (b, nw, k, c, hw)
FOLD_K = (0, 1, 2, 4)
FOLD_NW = (1, 2, 7)
FOLD_EXTRA = (0, 1, 5)


def fold_cases():
    return [(2, nw, k, 3, 5) for k in FOLD_K for nw in FOLD_NW]


# 65 536 blocks x 256 threads = 16 777 216 elements per trip; 16 777 219 = 1549 x 10831 (both prime)
FOLD_CAP = 65536 * 256
FOLD_BIG = dict(fold=(1, 1547, 1, 1, 10831),            # L = 1549
                fold_adjoint=(1, 1, 774, 1, 10831),     # one window of 1549 slots: the first and the last window at once
                unfold_adjoint=(1, 1547, 1, 1, 10831))


def fold_inputs(b, nw, k, c, hw, extra=0, seed=0):
    """s [b][nw][(2k+1) c][hw], g [b][L][c][hw], gwin [b][nw][(2k+1) c + extra][hw] whose extra channels are NaN"""
    g = torch.Generator().manual_seed(900 + 100 * k + 10 * nw + extra + seed)
    wc = (2 * k + 1) * c
    gwin = torch.full((b, nw, wc + extra, hw), float('nan'))
    gwin[:, :, :wc] = torch.randn(b, nw, wc, hw, generator=g)
    return dict(s=torch.randn(b, nw, wc, hw, generator=g), g=torch.randn(b, nw + 2 * k, c, hw, generator=g), gwin=gwin)


# ---- PC / guidance: one element, both sides of one workgroup, 8192 blocks x 256 threads + 5
PC_CAP = 8192 * 256
PC_NUMEL = (1, 255, 256, 257, PC_CAP + 5)
CORRECT_CAP = 2048 * 256
CORRECT_PER = (3, 4097, CORRECT_CAP + 3)
CORRECT_B = (1, 3)
MU, SIGMA, STD, GAMMA, R, C1, TAU = 0.83, 0.41, 0.37, 1e-2, 1.25, -0.37, 0.5


def pc_inputs(numel, seed=0):
    g = torch.Generator().manual_seed(4000 + numel % 9973 + seed)
    return [torch.randn(numel, generator=g) for _ in range(3)]


SUMSQ_NCHUNK = (1, 2, 7, 64, 1024)
SUMSQ_PER = (5, 4096, 65541)

# ---- time embedding: (nf, hidden, e); 2 nf = 128 is the LDS limit, hidden = 1024 and e = 300 take four and two trips of the thread loops
TE_SHAPES = ((1, 1, 1), (13, 100, 24), (32, 256, 64), (64, 1024, 300))
TE_NT = (1, 7)


def te_inputs(nf, hidden, e, nt):
    g = torch.Generator().manual_seed(100000 * nf + 100 * hidden + e)

    def uni(*shape, fan):
        return (torch.rand(*shape, generator=g) * 2 - 1) / math.sqrt(fan)
    p = dict(freqs=(torch.pi * torch.arange(1, nf + 1)).float(), w0=uni(hidden, 2 * nf, fan=2 * nf), b0=uni(hidden, fan=2 * nf),
             w2=uni(e, hidden, fan=hidden), b2=uni(e, fan=hidden))
    p['t'] = torch.tensor([0.37]) if nt == 1 else torch.tensor([0.0, 1.0, 0.5, 0.013, 0.987, 0.25, 0.8125])[:nt]
    return p


# ---- sda_linear_small: (rows, out_f) with rows x out_f = 1, 5, 2100, 2101 (a ragged last workgroup of 1 wave); in_f around one wavefront
LS_IN = (1, 63, 64, 65, 200)
LS_ROWS_OUT = ((1, 1), (5, 1), (7, 300), (11, 191))


def ls_inputs(rows, in_f, out_f):
    g = torch.Generator().manual_seed(rows * 1000 + in_f * 7 + out_f)
    return dict(x=torch.randn(rows, in_f, generator=g), w=torch.randn(out_f, in_f, generator=g) / math.sqrt(in_f),
                b=torch.randn(out_f, generator=g))


# ---- sda_vp_schedule
ETA = 1e-3
VP_K = (0.0, math.acos(math.sqrt(ETA)), math.log(ETA))
VP_T = (0.0, 1e-3, 0.5, 1 - 1e-3, 1.0)
