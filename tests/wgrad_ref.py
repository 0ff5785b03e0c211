"""Layer cases for the weight-gradient kernel (csrc/conv_wgrad.hip) and their float64 reference.

Each case builds one convolution's input the way its forward launch reads it (source view, context channels, modulation +
LayerNorm, activation, up-sampling), an output cotangent, and the float64 gradient torch.autograd forms for the conv's
weight and bias over the transformed input (oracle's ``layer_norm`` / ``activation`` / ``_conv``).  The same cases run on the
host emulator (test_wgrad_emulator.py) and on the device (test_gpu_training.py)."""
import ctypes

import torch

from oracle import sda_oracle as O
from sda_amd._lib import ACT_IDS, WgradDesc
from sda_amd.ops import conv_out_size, make_conv_desc

KINDS = ('plain', 'conv1', 'conv1_shared', 'conv2', 'tail_up', 'head_s2', 'head0_ctx', 'head0_window', 'tail10')


def _stats(v):
    """fp32 (mean, rstd) over channels of v (n, c, h, w), as the LayerNorm statistics kernel forms them (fp64 here)."""
    v = v.double()
    c = v.shape[1]
    mean = v.mean(dim=1)
    var = (v - mean[:, None]).square().sum(dim=1) / (c - 1 if O.LN_UNBIASED else c)
    return mean.float().reshape(-1).contiguous(), (1.0 / torch.sqrt(var + O.LN_EPS)).float().reshape(-1).contiguous()


def make_case(kind, dev, *, cin=8, cout=8, n=2, h=6, w=6, k=3, circular=True, one_d=False, act='SiLU', seed=0, ksize=None, pad=None,
              n_off=0):
    """-> dict(conv=ConvDesc, g, keep, v64 (the conv's virtual input, float64, (n, cin_total, hv, wv)), stride, circular, kh, kw).
    ksize: (kh, kw) instead of k x k; pad: explicit (pad_h, pad_w) instead of k // 2; n_off ('head0_window'): the layer reads the
    windows from n_off on (a recomputed chunk's view of the trajectory)."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    kh, kw = (1, k) if one_d else (k, k)
    if ksize is not None:
        kh, kw = ksize
    if one_d:
        h = 1
    keep = []
    stride = (1, 1)
    up = (1, 1)
    extra = {}
    if kind == 'head0_window':
        B, C, order = 2, max(1, cin // 3), 1
        wl = 2 * order + 1
        L = 4
        X = rnd(B, L, C, h, w)
        nw = L - 2 * order
        cx = wl * C
        n = B * nw - n_off
        ctx = rnd(1, h, w)
        x = X.to(dev)
        cx_tot = cx + 1
        v = torch.stack([X[b, i:i + wl].reshape(cx, h, w) for b in range(B) for i in range(nw)])[n_off:]
        v = torch.cat([v, ctx.expand(n, 1, h, w)], dim=1)
        ctxd = ctx.reshape(-1).contiguous().to(dev)
        keep += [x, ctxd]
        src = dict(x_ptr=x.data_ptr(), n=n, cx=cx, hs=h, ws=w, x_sn_outer=L * C * h * w, x_sn_inner=C * h * w, n_inner=nw,
                   x_n_off=n_off, x_sc=h * w, x_sy=w, x_sx=1)
        extra = dict(ctx_ptr=ctxd.data_ptr(), cctx=1, ctx_sn=0)
        cin = cx_tot
    elif kind == 'head0_ctx':
        a = rnd(n, cin - 1, h, w)
        ctx = rnd(1, h, w)
        x = a.to(dev)
        ctxd = ctx.reshape(-1).contiguous().to(dev)
        keep += [x, ctxd]
        v = torch.cat([a, ctx.expand(n, 1, h, w)], dim=1)
        src = dict(x_ptr=x.data_ptr(), n=n, cx=cin - 1, hs=h, ws=w, x_sn_outer=(cin - 1) * h * w, x_sc=h * w, x_sy=w, x_sx=1)
        extra = dict(ctx_ptr=ctxd.data_ptr(), cctx=1, ctx_sn=0)
    else:
        a = rnd(n, cin, h, w) * 1.5 + 0.3
        x = a.to(dev)
        keep.append(x)
        src = dict(x_ptr=x.data_ptr(), n=n, cx=cin, hs=h, ws=w, x_sn_outer=cin * h * w, x_sc=h * w, x_sy=w, x_sx=1)
        if kind in ('plain', 'tail10'):
            v = a
        elif kind in ('conv1', 'conv1_shared'):
            mod = rnd(1 if kind == 'conv1_shared' else n, cin)
            vin = a + mod[:, :, None, None]
            mean, rstd = _stats(vin)
            md, mn, rs = mod.to(dev).contiguous(), mean.to(dev), rstd.to(dev)
            keep += [md, mn, rs]
            extra = dict(mod_ptr=md.data_ptr(), mod_sn=0 if kind == 'conv1_shared' else cin, ln_mean_ptr=mn.data_ptr(),
                         ln_rstd_ptr=rs.data_ptr())
            v = O.layer_norm(vin.double(), dim=1)
        elif kind == 'conv2':
            extra = dict(act_in=ACT_IDS[act])
            v = O.activation(act)(a.double())
        elif kind == 'tail_up':
            mean, rstd = _stats(a)
            mn, rs = mean.to(dev), rstd.to(dev)
            keep += [mn, rs]
            extra = dict(ln_mean_ptr=mn.data_ptr(), ln_rstd_ptr=rs.data_ptr())
            up = (1, 2) if one_d else (2, 2)
            v = O.layer_norm(a.double(), dim=1)
            v = v.repeat_interleave(up[1], dim=3).repeat_interleave(up[0], dim=2)
        elif kind == 'head_s2':
            stride = (1, 2) if one_d else (2, 2)
            v = a
        else:
            raise ValueError(kind)
    hv, wv = v.shape[2], v.shape[3]
    ho, wo = conv_out_size(hv, kh, stride[0]), conv_out_size(wv, kw, stride[1])
    if pad is not None:
        ho, wo = (hv + 2 * pad[0] - kh) // stride[0] + 1, (wv + 2 * pad[1] - kw) // stride[1] + 1
    g = rnd(n, cout, ho, wo).to(dev).contiguous()
    conv = make_conv_desc(pad=pad, **src, w_ptr=0, cin_pad=0, cout_pad=0, cout=cout, kh=kh, kw=kw, out_ptr=0, ho=ho, wo=wo, mt=1,
                          stride_h=stride[0], stride_w=stride[1], circular=circular, up_h=up[0], up_w=up[1], **extra)
    return dict(conv=conv, g=g, keep=keep, v64=v.double(), stride=stride, circular=circular, kh=kh, kw=kw, cin=cin, cout=cout,
                one_d=one_d, pad=pad)


def reference(case):
    """float64 (dW, db) of torch.autograd over the case's transformed input (oracle._conv: padding k//2, zeros | circular)."""
    v = case['v64']
    cout, cin, kh, kw = case['cout'], v.shape[1], case['kh'], case['kw']
    g = case['g'].detach().double().cpu()
    if case.get('pad') is not None:
        return reference_general(v, g, cout, kh, kw, case['stride'], case['circular'], case['pad'])
    W = torch.zeros(cout, cin, kh, kw, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    mode = 'circular' if case['circular'] else 'zeros'
    if case['one_d']:
        out = O._conv(v[:, :, 0], W[:, :, 0], b, 1, case['stride'][1], mode)
        dW, db = torch.autograd.grad(out, (W, b), g[:, :, 0])
    else:
        out = O._conv(v, W, b, 2, case['stride'], mode)
        dW, db = torch.autograd.grad(out, (W, b), g)
    return dW, db


def wgrad_desc(case, dw, db, work=None, slabs=0, accumulate=False):
    d = WgradDesc()
    d.conv = case['conv']
    d.g, d.dw, d.db = case['g'].data_ptr(), dw.data_ptr(), None if db is None else db.data_ptr()
    d.work = 1 if work is None else work.data_ptr()
    d.slabs, d.accumulate = slabs, int(accumulate)
    return d


def work_floats(lib, d) -> int:
    return int(lib.sda_conv_wgrad_work_floats(ctypes.byref(d)))


def reference_general(v64, g64, cout, kh, kw, stride, circular, pad=None):
    """float64 (dW, db) for a 2-D layer over the virtual input ``v64`` (n, cin, hv, wv) with any (kh, kw) and stride.  ``pad``
    None: the oracle's convolution (padding k // 2).  ``pad`` = (ph, pw): the explicit padding of the descriptor, applied by
    hand (zeros or wrap-around) in front of a valid convolution."""
    import torch.nn.functional as F
    W = torch.zeros(cout, v64.shape[1], kh, kw, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    if pad is None:
        out = O._conv(v64, W, b, 2, tuple(stride), 'circular' if circular else 'zeros')
    else:
        ph, pw = pad
        vp = F.pad(v64, (pw, pw, ph, ph), mode='circular') if circular else F.pad(v64, (pw, pw, ph, ph))
        out = F.conv2d(vp, W, b, stride=tuple(stride))
    assert out.shape == g64.shape, (tuple(out.shape), tuple(g64.shape))
    return torch.autograd.grad(out, (W, b), g64)
