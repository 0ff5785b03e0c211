"""Float64 torch reference of the one-launch residual block of the 1-D nets (csrc/block1d.hip, sda/nn.py:18-28 of the reference with
spatial = 1), written from the operation, not from the kernel's tiling:

    xh   = (x - mean_c(x)) * rstd,  x = a + mod,  rstd = 1 / sqrt(var_c(x) + eps)      per position, over the channels
    z    = conv1(xh) + b1                                                              k = 3, stride 1, zero or circular padding
    y    = a + conv2(act(z)) + b2
    gx   = d <y, g> / d a                                                              (autograd of the above)
"""
import torch
import torch.nn.functional as F

ACTS = {'SiLU': F.silu, 'ReLU': F.relu, 'ELU': F.elu, 'GELU': F.gelu, 'SELU': F.selu}


def _conv3(x, w, b, circular):
    """x: (n, c, len), w: (c, c, 3): `same` cross-correlation with zero or circular padding, out[l] = sum_k w[:, :, k] x[l - 1 + k]."""
    length = x.shape[-1]
    xp = torch.cat([x[..., -1:], x, x[..., :1]], dim=-1) if circular else F.pad(x, (1, 1))
    out = sum(torch.einsum('oi,nil->nol', w[:, :, k], xp[..., k:k + length]) for k in range(3))
    return out if b is None else out + b[None, :, None]


def block1d_forward(a, mod, w1, b1, w2, b2, circular, act, eps, unbiased):
    """a: (n, c, len); mod: None, (1, c) (shared) or (n, c).  Returns y, z (n, c, len) and mean, rstd (n, len), all float64."""
    a, w1, w2 = a.double(), w1.double(), w2.double()
    b1 = None if b1 is None else b1.double()
    b2 = None if b2 is None else b2.double()
    x = a if mod is None else a + mod.double()[:, :, None]
    c = x.shape[1]
    mean = x.mean(dim=1)
    cen = x - mean[:, None]
    var = cen.square().sum(dim=1) / (c - 1 if unbiased else c)
    rstd = 1.0 / torch.sqrt(var + eps)
    z = _conv3(cen * rstd[:, None], w1, b1, circular)
    y = a + _conv3(ACTS[act](z), w2, b2, circular)
    return y, z, mean, rstd


def block1d_reference(a, mod, w1, b1, w2, b2, g, circular, act, eps, unbiased):
    """The five outputs of sda_block1d_fwd + sda_block1d_bwd in float64 (CPU): dict y, z, mean, rstd, gx."""
    a64 = a.detach().cpu().double().requires_grad_(True)
    cpu = lambda t: None if t is None else t.detach().cpu()
    y, z, mean, rstd = block1d_forward(a64, cpu(mod), cpu(w1), cpu(b1), cpu(w2), cpu(b2), circular, act, eps, unbiased)
    gx, = torch.autograd.grad(y, a64, cpu(g).double())
    return dict(y=y.detach(), z=z.detach(), mean=mean.detach(), rstd=rstd.detach(), gx=gx)
