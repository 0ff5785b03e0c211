"""TEST-ONLY reference of the keyed denoising loss (sda_amd/csrc/train_loss.hip): the times and the noise of a training step rebuilt
from tests/philox_ref.py, the loss and its cotangent in float64, the error bounds of sda_loss_mse from its launch geometry, and the
small nets / the uncaptured keyed training step the graph tests compare against."""
import math

import numpy as np
import torch

from tests import philox_ref as P

# the documented geometry of sda_loss_mse (include/sda_hip.h): chunks of 4096 elements, 16 terms per thread, a 6 + 3 tree per workgroup,
# 256 threads in stage 2
MSE_CHUNK, MSE_PER_THREAD, MSE_TREE, MSE_THREADS = 4096, 16, 9, 256


def t_rows(rows, seed, row0, step):
    """t[b] = ((w0 >> 8) + 0.5) 2^-24, w0 = word 0 at quad 0 of row row0 + b in draw 2 step + 1 -> float32 (rows,)."""
    draw = 2 * step + 1
    grow = np.arange(rows, dtype=np.uint64) + np.uint64(row0)
    c3 = (np.uint64(draw >> 32) ^ ((grow >> np.uint64(32)) << np.uint64(24))) & P.MASK
    w0 = P.philox4x32_10(np.uint64(0), grow & P.MASK, np.uint64(draw & 0xffffffff), c3, seed & 0xffffffff, (seed >> 32) & 0xffffffff)[0]
    return ((w0 >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def eps_rows(rows, per_row, seed, row0, step):
    """The noise of the step as the numpy restatement forms it (float round-off from the device: the bitwise yardstick is ops.randn_rows)."""
    return P.randn_rows(rows, per_row, seed, row0, 2 * step)


def mse64(out, eps):
    """float64 (loss, cotangent at out) of mean((out - eps)^2) from fp32 tensors."""
    d = out.detach().double().cpu() - eps.detach().double().cpu()
    return float((d * d).mean()), 2.0 * d / d.numel()


def mse_chain(numel):
    """(workgroups of stage 1, the longest chain of additions a term passes through) from the documented geometry."""
    blocks = -(-numel // MSE_CHUNK)
    return blocks, MSE_PER_THREAD + MSE_TREE + -(-blocks // MSE_THREADS) + MSE_TREE


def k_of(alpha_kind, eta):
    return (0.0, math.acos(math.sqrt(eta)), math.log(eta))[alpha_kind]
