#!/usr/bin/env python3
"""Randomised parity sweep of the weight-gradient kernel (csrc/conv_wgrad.hip) against float64 torch.autograd, on the device or
on its host emulator (libsda_emu.so).

    python tests/fuzz/wgrad_fuzz.py [--cases 300] [--seed 0] [--emu]

Every case draws one layer descriptor: the source view (planar, channel-last, or the sliding-window view of a trajectory with an
image offset into it), context channels (shared or per image), one of the loader modes (plain, modulation + LayerNorm with a
shared or per-image row, LayerNorm alone, one of the five activations, nearest up-sample, stride), kernel sizes 1..7 with
kh != kw, explicit padding, circular or zero padding, every cout tile incl. ragged last ones, a slab count, accumulation onto a
prior gradient, bias gradient present or absent.  The reference builds the layer's virtual input in float64 by plain indexing
and differentiates the oracle's convolution; it shares no index helper with the kernel.  Tolerance 1e-5 of max |ref|."""
import argparse
import ctypes
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from oracle import sda_oracle as O  # noqa: E402
from sda_amd._lib import ACT_IDS, WgradDesc  # noqa: E402
from sda_amd.ops import make_conv_desc  # noqa: E402
from tests.wgrad_ref import reference_general  # noqa: E402

TOL = 1e-5
MODES = ('plain', 'mod_ln', 'ln', 'act', 'up', 'stride')
COUTS = (1, 5, 10, 31, 32, 33, 64, 96, 97, 100, 130)


class Backend:
    """Where a case runs: ``emulator()`` (host tensors through libsda_emu.so) or ``device()`` (cuda:0 through libsda_hip.so)."""

    def __init__(self, lib, dev, launch):
        self.lib, self.dev, self.launch = lib, torch.device(dev), launch

    def work_floats(self, d) -> int:
        return int(self.lib.sda_conv_wgrad_work_floats(ctypes.byref(d)))


def emulator() -> Backend:
    from sda_amd import build as sbuild
    lib = ctypes.CDLL(sbuild.build_emu())
    lib.sda_conv_wgrad_emulate.restype = ctypes.c_int
    lib.sda_conv_wgrad_emulate.argtypes = [ctypes.POINTER(WgradDesc)]
    lib.sda_conv_wgrad_work_floats.restype = ctypes.c_int64
    lib.sda_conv_wgrad_work_floats.argtypes = [ctypes.POINTER(WgradDesc)]
    return Backend(lib, 'cpu', lambda d: int(lib.sda_conv_wgrad_emulate(ctypes.byref(d))))


def device() -> Backend:
    from sda_amd._lib import load
    lib = load()

    def launch(d):
        rc = int(lib.sda_conv_wgrad(ctypes.byref(d), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc
    return Backend(lib, 'cuda:0', launch)


def draw_case(rng, idx):
    """-> spec: the host tensors of one layer, its descriptor fields (tensors by name) and the float64 virtual input."""
    gen = torch.Generator().manual_seed(77000 + idx)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    one_d = rng.random() < 0.3
    h = 1 if one_d else rng.choice([1, 3, 4, 5, 6, 8])
    w = rng.choice([3, 4, 5, 6, 8, 12])
    circ = rng.random() < 0.5
    window = rng.random() < 0.4
    chan_last = (not window) and rng.random() < 0.3
    cctx = rng.choice([0, 0, 1, 2, 3])
    ctx_per_image = bool(cctx) and rng.random() < 0.5
    cout = rng.choice(COUTS)
    mode = rng.choice(MODES)
    up, stride = (1, 1), (1, 1)
    if mode == 'up':
        up = (1, 2) if one_d or rng.random() < 0.3 else (2, 2)
    if mode == 'stride':
        stride = (1, 2) if one_d or rng.random() < 0.3 else (2, 2)
    hv, wv = h * up[0], w * up[1]
    explicit = rng.random() < 0.25
    if explicit:                                 # any kernel size (even ones too), any pad below it
        kh = 1 if one_d else rng.choice([1, 2, 3, 4, 5])
        kw = rng.choice([1, 2, 3, 4, 5, 7])
        pad = (rng.randrange(kh), rng.randrange(kw))
    else:
        kh = 1 if one_d else rng.choice([1, 3, 3, 5])
        kw = rng.choice([1, 3, 3, 5, 7])
        pad = (kh // 2, kw // 2)
    if circ and (pad[0] > hv or pad[1] > wv):    # (the oracle's circular padding needs pad <= size)
        circ = False
    if hv + 2 * pad[0] < kh or wv + 2 * pad[1] < kw:
        explicit, pad = False, (kh // 2, kw // 2)
        if not (kh & 1):
            kh += 1
            pad = (kh // 2, pad[1])
        if not (kw & 1):
            kw += 1
            pad = (pad[0], kw // 2)
        if circ and (pad[0] > hv or pad[1] > wv):
            circ = False
    T = {}                                       # host tensors by name
    if window:
        B, L, C = rng.choice([1, 2, 3]), rng.choice([3, 4, 6]), rng.choice([1, 2, 3])
        wl = 3
        nw, cx = L - wl + 1, wl * C
        ntot = B * nw
        T['x'] = rnd(B, L, C, h, w)
        full = torch.stack([T['x'][b, i:i + wl].reshape(cx, h, w) for b in range(B) for i in range(nw)])
        lo = rng.randrange(ntot)
        n = rng.randint(1, ntot - lo)
        src = dict(n=n, cx=cx, hs=h, ws=w, x_sn_outer=L * C * h * w, x_sn_inner=C * h * w, n_inner=nw, x_n_off=lo, x_sc=h * w,
                   x_sy=w, x_sx=1)
    else:
        ntot, cx = rng.choice([1, 2, 3, 5]), rng.choice([1, 3, 7, 9, 16, 43])
        lo = rng.randrange(ntot)
        n = rng.randint(1, ntot - lo)
        if chan_last:
            T['x'] = rnd(ntot, h, w, cx)
            full = T['x'].permute(0, 3, 1, 2)
            src = dict(n=n, cx=cx, hs=h, ws=w, x_sn_outer=h * w * cx, x_n_off=lo, x_sc=1, x_sy=w * cx, x_sx=cx)
        else:
            T['x'] = rnd(ntot, cx, h, w)
            full = T['x']
            src = dict(n=n, cx=cx, hs=h, ws=w, x_sn_outer=cx * h * w, x_n_off=lo, x_sc=h * w, x_sy=w, x_sx=1)
    a = full[lo:lo + n].double()
    ptrs, extra = {}, {}                         # descriptor pointer fields -> tensor names; plain fields
    shared = None
    if mode == 'mod_ln':
        shared = rng.random() < 0.5
        T['mod'] = rnd(1 if shared else n, cx)
        a = a + T['mod'].double()[:, :, None, None]
        ptrs['mod_ptr'] = 'mod'
        extra['mod_sn'] = 0 if shared else cx
    if mode in ('mod_ln', 'ln', 'up') and cx > 1:
        mean = a.mean(1)
        var = (a - mean[:, None]).square().sum(1) / (cx - 1 if O.LN_UNBIASED else cx)
        T['mean'] = mean.float().reshape(-1).contiguous()
        T['rstd'] = (1 / torch.sqrt(var + O.LN_EPS)).float().reshape(-1).contiguous()
        ptrs.update(ln_mean_ptr='mean', ln_rstd_ptr='rstd')
        a = (a - T['mean'].double().reshape(n, 1, h, w)) * T['rstd'].double().reshape(n, 1, h, w)
    v = a
    if cctx:
        T['ctx'] = rnd(n if ctx_per_image else 1, cctx, h, w)
        ptrs['ctx_ptr'] = 'ctx'
        extra.update(cctx=cctx, ctx_sn=cctx * h * w if ctx_per_image else 0)
        v = torch.cat([v, T['ctx'].double().expand(n, cctx, h, w)], 1)
    act = None
    if mode == 'act':
        act = rng.choice(['SiLU', 'ReLU', 'ELU', 'GELU', 'SELU'])
        extra['act_in'] = ACT_IDS[act]
        v = O.activation(act)(v)
    v = v.repeat_interleave(up[1], 3).repeat_interleave(up[0], 2)
    ho = (hv + 2 * pad[0] - kh) // stride[0] + 1
    wo = (wv + 2 * pad[1] - kw) // stride[1] + 1
    cin = cx + cctx
    T['g'] = rnd(n, cout, ho, wo).contiguous()
    accumulate = rng.random() < 0.4
    with_db = rng.random() < 0.75
    T['dw'] = rnd(cout, cin, kh, kw) * 3 if accumulate else torch.full((cout, cin, kh, kw), float('nan'))
    T['db'] = rnd(cout) * 3 if accumulate else torch.full((cout,), float('nan'))
    slabs = rng.choice([0, 1, 3, 64])
    cfg = dict(idx=idx, one_d=one_d, h=h, w=w, kh=kh, kw=kw, pad=pad if explicit else None, circ=circ, window=window,
               chan_last=chan_last, cctx=cctx, ctx_per_image=ctx_per_image, cx=cx, cout=cout, mode=mode, act=act, shared=shared,
               up=up, stride=stride, n=n, lo=lo, slabs=slabs, accumulate=accumulate, with_db=with_db)
    desc = dict(src, cout=cout, kh=kh, kw=kw, ho=ho, wo=wo, stride_h=stride[0], stride_w=stride[1], circular=circ, up_h=up[0],
                up_w=up[1], pad=pad if explicit else None, **extra)
    return dict(cfg=cfg, T=T, desc=desc, ptrs=ptrs, v64=v, pad=pad, stride=stride, circ=circ, slabs=slabs, accumulate=accumulate,
                with_db=with_db)


def run_case(spec, backend):
    """One launch of ``spec`` on ``backend`` -> (dw, db or None, None) as host tensors, or (None, None, message)."""
    dev = backend.dev
    D = {k: t.to(dev) for k, t in spec['T'].items()}
    conv = make_conv_desc(x_ptr=D['x'].data_ptr(), w_ptr=0, cin_pad=0, cout_pad=0, out_ptr=0, mt=1,
                          **{k: D[name].data_ptr() for k, name in spec['ptrs'].items()}, **spec['desc'])
    dw, db = D['dw'].clone(), D['db'].clone()
    d = WgradDesc()
    d.conv = conv
    d.g, d.dw, d.db = D['g'].data_ptr(), dw.data_ptr(), db.data_ptr() if spec['with_db'] else None
    d.work = 1                                   # (placeholder for planning)
    d.slabs, d.accumulate = spec['slabs'], int(spec['accumulate'])
    floats = backend.work_floats(d)
    if floats <= 0:                              # nothing is launched for a descriptor the planner refuses
        return None, None, f'the planner refused the descriptor: rc {floats}'
    work = torch.full((floats,), float('nan'), device=dev)     # (an unwritten slab would show)
    d.work = work.data_ptr()
    rc = backend.launch(d)
    if rc != 0:
        return None, None, f'launch rc {rc}'
    if not spec['with_db'] and not torch.equal(db.cpu().isnan(), spec['T']['db'].isnan()):
        return None, None, 'db written although no bias gradient was asked for'
    if not spec['with_db'] and spec['accumulate'] and not torch.equal(db.cpu(), spec['T']['db']):
        return None, None, 'db changed although no bias gradient was asked for'
    return dw.cpu(), db.cpu() if spec['with_db'] else None, None


def reference(spec):
    """float64 (dW, db) incl. the prior when accumulating, and the scales max |dW|, max |db| of the gradient alone."""
    cout, kh, kw = spec['desc']['cout'], spec['desc']['kh'], spec['desc']['kw']
    rw, rb = reference_general(spec['v64'], spec['T']['g'].double(), cout, kh, kw, spec['stride'], spec['circ'],
                               spec['pad'] if spec['desc']['pad'] is not None else None)
    sw, sb = rw.abs().max().item() + 1e-30, rb.abs().max().item() + 1e-30
    if spec['accumulate']:
        rw, rb = rw + spec['T']['dw'].double(), rb + spec['T']['db'].double()
    return rw, rb, sw, sb


def errors(spec, dw, db, ref=None):
    rw, rb, sw, sb = ref or reference(spec)
    ew = (dw.double() - rw).abs().max().item() / sw
    eb = 0.0 if db is None else (db.double() - rb).abs().max().item() / sb
    return ew, eb


def one_case(rng, backend, idx):
    spec = draw_case(rng, idx)
    cfg = spec['cfg']
    dw, db, msg = run_case(spec, backend)
    if msg:
        return cfg, msg
    if not torch.isfinite(dw).all() or (db is not None and not torch.isfinite(db).all()):
        return cfg, 'non-finite gradient'
    ew, eb = errors(spec, dw, db)
    if not (ew <= TOL and eb <= TOL):
        return cfg, f'dw err {ew:.3e}, db err {eb:.3e} (relative to max |ref|; bound {TOL:g})'
    return cfg, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', type=int, default=300)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--emu', action='store_true', help='run on the host emulator (no GPU needed)')
    args = ap.parse_args()
    rng = random.Random(args.seed)
    backend = emulator() if args.emu else device()
    bad = 0
    for i in range(args.cases):
        cfg, msg = one_case(rng, backend, i + 7919 * args.seed)
        if msg:
            bad += 1
            print(f'FAIL case {i}: {msg}\n     {cfg}', flush=True)
    print(f'{args.cases - bad}/{args.cases} layer weight gradients within {TOL:g} of float64 '
          f'({"host emulator" if args.emu else "device"})')
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
