"""Shared by tests/test_adamw_host.py (the host emulator) and tests/test_gpu_adamw.py (the device): descriptor filling for
sda_adamw_step, the pack shapes, the five-step arithmetic case, its float64 replay and the tolerance rule."""
import ctypes
import math

import torch

from sda_amd import _lib, mlp
from sda_amd import build as sbuild

BETAS, EPS, WD = (0.9, 0.999), 1e-8, 1e-3
LRS = (1e-3, 3e-3, 1e-2, 5e-4, 2e-3)                     # one per step: the learning rate changes each step
SIZES = (1, 5, 1023, 4100)                               # below one float4, odd, one short of a chunk (scalar path), four chunks + 1 float4
SCALES = (1.0, 1e-3)
# (in_f, out_f): every padding class of _mf (16 / 128 / 256) and _kq (16 / 64 / 128 / 256); one-, two- and four-unit slabs
PACK_SHAPES = ((3, 5), (15, 15), (16, 16), (47, 256), (256, 15), (256, 256), (17, 129), (64, 128), (65, 17), (128, 129))


def load_emu():
    """libsda_emu.so with the host replay of the step bound."""
    lib = ctypes.CDLL(sbuild.build_emu())
    lib.sda_adamw_step_emulate.restype = ctypes.c_int
    lib.sda_adamw_step_emulate.argtypes = [ctypes.POINTER(_lib.AdamWDesc)]
    return lib


def hyper(d, lr, wd, t, betas=BETAS, eps=EPS):
    """The scalars of the descriptor for step t (formed in double, stored as fp32), as sda_amd.training.AdamW forms them."""
    b1, b2 = betas
    d.decay, d.one_m_beta1, d.beta2, d.one_m_beta2 = 1.0 - lr * wd, 1.0 - b1, b2, 1.0 - b2
    d.step_size, d.rsqrt_bc2, d.eps = lr / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t), eps
    return d


def desc(tensors, lr, wd, t):
    """tensors: [(p, g, m, v) or (p, g, m, v, kind, out_f, in_f, fwd, bwd)] of contiguous fp32 tensors (host or device)."""
    d = hyper(_lib.AdamWDesc(), lr, wd, t)
    d.ntensor = len(tensors)
    for n, (p, g, m, v, *pack) in enumerate(tensors):
        d.p[n], d.g[n], d.m[n], d.v[n], d.numel[n] = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
        if pack:
            kind, out_f, in_f, fwd, bwd = pack
            d.pack_kind[n], d.out_f[n], d.in_f[n] = kind, out_f, in_f
            d.fwd[n], d.bwd[n] = fwd.data_ptr(), None if bwd is None else bwd.data_ptr()
    return d


def pack_case(in_f, out_f, device='cpu'):
    """A weight [out_f][in_f] with distinct entries, a bias, zeroed state and zeroed destinations of the slab sizes _FusedPlan._pack uses."""
    W = (torch.arange(out_f * in_f, dtype=torch.float32) + 1).reshape(out_f, in_f).to(device)
    b = (torch.arange(out_f, dtype=torch.float32) + 0.5).to(device)
    size = max(mlp._slab(W).numel(), mlp._slab(W.t()).numel())
    return dict(W=W, b=b, gW=torch.linspace(-1, 1, W.numel(), device=device).reshape(out_f, in_f).contiguous(), gb=torch.linspace(-1, 1, out_f, device=device),
                mW=torch.zeros_like(W), vW=torch.zeros_like(W), mb=torch.zeros_like(b), vb=torch.zeros_like(b),
                fwd=torch.zeros(size, device=device), bwd=torch.zeros(size, device=device), bias=torch.zeros(16 * mlp._mf(out_f), device=device))


def pack_desc(c, lr, wd, t=1):
    out_f, in_f = c['W'].shape
    return desc([(c['W'], c['gW'], c['mW'], c['vW'], 1, out_f, in_f, c['fwd'], c['bwd']),
                 (c['b'], c['gb'], c['mb'], c['vb'], 2, out_f, 0, c['bias'], None)], lr, wd, t)


def check_pack(c):
    """The destinations equal, bitwise and padding included, the slabs the host packer forms from the (updated) parameter."""
    W, b = c['W'], c['b']
    sf, sb = mlp._slab(W), mlp._slab(W.t())
    assert torch.equal(c['fwd'][:sf.numel()], sf) and (c['fwd'][sf.numel():] == 0).all()
    assert torch.equal(c['bwd'][:sb.numel()], sb) and (c['bwd'][sb.numel():] == 0).all()
    assert torch.equal(c['bias'][:b.numel()], b) and (c['bias'][b.numel():] == 0).all()


def arithmetic_inputs(scale, seed=0):
    """Parameters N(0, 1) of SIZES elements and five gradients each: N(0, 1) * scale with a tenth of the entries exactly 0."""
    gen = torch.Generator().manual_seed(seed)
    params = [torch.randn(n, generator=gen) for n in SIZES]
    grads = []
    for _ in LRS:
        step = []
        for n in SIZES:
            g = torch.randn(n, generator=gen) * scale
            g[torch.rand(n, generator=gen) < 0.1] = 0.0
            step.append(g)
        grads.append(step)
    return params, grads


def emulate_five_steps(emu, params, grads):
    """The arithmetic case through the host emulator -> per tensor (p, m, v)."""
    ps = [p.clone() for p in params]
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    for t, lr in enumerate(LRS, start=1):
        d = desc(list(zip(ps, grads[t - 1], ms, vs)), lr, WD, t)
        assert emu.sda_adamw_step_emulate(ctypes.byref(d)) == 0
    return list(zip(ps, ms, vs))


def replay64(params, grads):
    """The update formula in float64 from the same fp32 start values -> per tensor (p, m, v) after the five steps."""
    b1, b2 = BETAS
    out = []
    for n, p0 in enumerate(params):
        p, m, v = p0.double().clone(), torch.zeros_like(p0, dtype=torch.float64), torch.zeros_like(p0, dtype=torch.float64)
        for t, lr in enumerate(LRS, start=1):
            g = grads[t - 1][n].double()
            p = p * (1 - lr * WD)
            m = m + (g - m) * (1 - b1)
            v = v * b2 + (1 - b2) * g * g
            p = p - (lr / (1 - b1 ** t)) * m / (v.sqrt() / math.sqrt(1 - b2 ** t) + EPS)
        out.append((p, m, v))
    return out


def torch_adamw(params, grads, device='cpu', **kw):
    """torch.optim.AdamW's single-tensor route on the same inputs -> per tensor (p, exp_avg, exp_avg_sq)."""
    ps = [torch.nn.Parameter(p.clone().to(device)) for p in params]
    opt = torch.optim.AdamW(ps, lr=LRS[0], betas=BETAS, eps=EPS, weight_decay=WD, foreach=False, **kw)
    for t, lr in enumerate(LRS):
        opt.param_groups[0]['lr'] = lr
        for p, g in zip(ps, grads[t]):
            p.grad = g.clone().to(device)
        opt.step()
    return [(p.detach().cpu(), opt.state[p]['exp_avg'].cpu(), opt.state[p]['exp_avg_sq'].cpu()) for p in ps]


def ulp(x):
    """One unit in the last place of fp32 at the magnitude max |x|."""
    a = float(x.abs().max())
    return 0.0 if a == 0.0 else 2.0 ** (math.floor(math.log2(a)) - 23)


def check_against_float64(got, yard, ref):
    """got / yard / ref: per tensor (p, m, v) of the code under test, of torch.optim.AdamW and of the float64 replay.  Two fp32
    implementations of one formula that round at different places differ from the exact result by a small factor of one another, not
    more: the maximum error of the code under test may be at most twice torch's own plus one ulp of the quantity.  Returns the worst
    (error, torch's error) of p over the tensors, for the record."""
    worst = (0.0, 0.0)
    for n, (g3, y3, r3) in enumerate(zip(got, yard, ref)):
        for name, g, y, r in zip('pmv', g3, y3, r3):
            err, err_t = float((g.double() - r).abs().max()), float((y.double() - r).abs().max())
            print(f'tensor {n} ({g.numel()} elements) {name}: max error to float64 {err:.3e}, torch.optim.AdamW {err_t:.3e}, ulp {ulp(r):.3e}')
            assert err <= 2 * err_t + ulp(r), (n, name, err, err_t, ulp(r))
            if name == 'p' and err > worst[0]:
                worst = (err, err_t)
    return worst
