#!/usr/bin/env python3
"""Randomised parity sweep of the heads' and tails' tiled weight-gradient kernel (csrc/conv_wgrad3.hip, sda_conv_wgrad3x) over its served set against
float64 torch.autograd, on the device or on its host replay (libsda_emu.so).

    python tests/fuzz/wgrad3x_fuzz.py [--cases 200] [--seed 0] [--emu]

Every case draws one served layer: the geometry (up-sampling tail with or without its LayerNorm, stride-2 head), cin in 32 {1, 2, 3},
cout in 32 {1 .. 6} (every cout tile, up to six of them), image counts and OUTPUT sizes on both sides of every planner threshold (one
row per stage from wo + 2 = 65, R (wo + 2) off the multiples of 4, ragged last row blocks, the one-pixel sources), circular or zero
padding, a forced or the planner's own slab count, accumulation onto a prior gradient, bias gradient present or absent.  The source
size follows from the output size (half of it for the tails: even outputs only; twice it for the heads), so every draw is served:
a draw the planner refuses is a failure.  The reference is tests/wgrad_ref.reference.  Tolerance 1e-5 of max |ref| (wgrad3_fuzz's)."""
import argparse
import ctypes
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from sda_amd._lib import WgradDesc  # noqa: E402
from tests import wgrad_ref  # noqa: E402
from tests.wgrad3x_cases import S2, UP2, UP2_PLAIN, make, plan  # noqa: E402

TOL = 1e-5
KINDS = (UP2, UP2_PLAIN, S2)
CINS = (32, 64, 96)
COUTS = (32, 64, 96, 128, 160, 192)
NS = (1, 2, 3, 300)
HOS = (1, 2, 3, 4, 6, 14)                       # output rows (the tails take the even ones)
WOS = (1, 2, 3, 4, 8, 12, 30, 32, 62, 63, 64, 66)
SLABS = (0, 1, 2, 3, 64)


class Backend:
    """Where a case runs: ``emulator()`` (host tensors through libsda_emu.so) or ``device()`` (cuda:0 through libsda_hip.so)."""

    def __init__(self, lib, dev, launch):
        self.lib, self.dev, self.launch = lib, torch.device(dev), launch
        lib.sda_conv_wgrad3x_work_floats.restype = ctypes.c_int64
        lib.sda_conv_wgrad3x_work_floats.argtypes = [ctypes.POINTER(WgradDesc)]

    def work_floats(self, d) -> int:
        return int(self.lib.sda_conv_wgrad3x_work_floats(ctypes.byref(d)))


def emulator() -> Backend:
    from sda_amd import build as sbuild
    lib = ctypes.CDLL(sbuild.build_emu())
    lib.sda_conv_wgrad3x_emulate.restype = ctypes.c_int
    lib.sda_conv_wgrad3x_emulate.argtypes = [ctypes.POINTER(WgradDesc)]
    return Backend(lib, 'cpu', lambda d: int(lib.sda_conv_wgrad3x_emulate(ctypes.byref(d))))


def device() -> Backend:
    from sda_amd._lib import load
    lib = load()

    def launch(d):
        rc = int(lib.sda_conv_wgrad3x(ctypes.byref(d), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc
    return Backend(lib, 'cuda:0', launch)


def draw_case(rng, idx):
    """-> spec: the layer's configuration (``cfg``, the planner's expected plan in it), the prior dw / db on the host, the layer
    itself built on the host (``case``: what the reference and the emulator read)."""
    kind = rng.choice(KINDS)
    cin, cout = rng.choice(CINS), rng.choice(COUTS)
    n = rng.choice(NS)
    if n == 300:                                 # (more stages than the planner makes slabs: tiny images, three cin tiles)
        cin, cout, ho, wo = 96, 32, rng.choice((1, 2)), rng.choice((1, 2))
    else:
        ho, wo = rng.choice(HOS), rng.choice(WOS)
    if kind == S2:
        h, w = 2 * ho, 2 * wo
    else:                                        # even outputs: round up
        h, w = (ho + 1) // 2, (wo + 1) // 2
    circ = rng.random() < 0.5
    slabs = rng.choice(SLABS)
    accumulate = rng.random() < 0.4
    with_db = rng.random() < 0.75
    gen = torch.Generator().manual_seed(88000 + idx)
    dw = torch.randn(cout, cin, 3, 3, generator=gen) * 3 if accumulate else torch.full((cout, cin, 3, 3), float('nan'))
    db = torch.randn(cout, generator=gen) * 3 if accumulate else torch.full((cout,), float('nan'))
    p = plan(kind, cin, cout, n, h, w, slabs)
    cfg = dict(idx=idx, kind=kind, cin=cin, cout=cout, n=n, h=h, w=w, circ=circ, slabs=slabs, accumulate=accumulate,
               with_db=with_db, plan={k: p[k] for k in ('R', 'nrb', 'mt', 'n_ct', 'n_cit', 'q4_rounds', 'per', 'slabs')})
    return dict(cfg=cfg, dw=dw, db=db, case=build_case(cfg, 'cpu'), slabs=slabs, accumulate=accumulate, with_db=with_db)


def build_case(cfg, dev):
    return make(cfg['kind'], dev, cin=cfg['cin'], cout=cfg['cout'], n=cfg['n'], h=cfg['h'], w=cfg['w'], circular=cfg['circ'],
                seed=99000 + cfg['idx'])


def run_case(spec, backend):
    """One launch of ``spec`` on ``backend`` -> (dw, db or None, None) as host tensors, or (None, None, message)."""
    dev = backend.dev
    case = spec['case'] if dev.type == 'cpu' else build_case(spec['cfg'], dev)
    dw, db = spec['dw'].to(dev).clone(), spec['db'].to(dev).clone()
    dbp = db if spec['with_db'] else None
    d = wgrad_ref.wgrad_desc(case, dw, dbp, slabs=spec['slabs'], accumulate=spec['accumulate'])
    floats = backend.work_floats(d)
    if floats <= 0:                              # nothing is launched for a descriptor the planner refuses
        return None, None, f'the planner refused the descriptor: rc {floats}'
    cfg = spec['cfg']
    if floats != cfg['plan']['slabs'] * cfg['cout'] * (cfg['cin'] * 9 + 1):
        return None, None, f'work size {floats} is not that of the expected plan'
    work = torch.full((floats,), float('nan'), device=dev)     # (an unwritten cell would show)
    d = wgrad_ref.wgrad_desc(case, dw, dbp, work, slabs=spec['slabs'], accumulate=spec['accumulate'])
    rc = backend.launch(d)
    if rc != 0:
        return None, None, f'launch rc {rc}'
    if not spec['with_db'] and not torch.equal(db.cpu().isnan(), spec['db'].isnan()):
        return None, None, 'db written although no bias gradient was asked for'
    if not spec['with_db'] and spec['accumulate'] and not torch.equal(db.cpu(), spec['db']):
        return None, None, 'db changed although no bias gradient was asked for'
    return dw.cpu(), db.cpu() if spec['with_db'] else None, None


def reference(spec):
    """float64 (dW, db) incl. the prior when accumulating, and the scales max |dW|, max |db| of the gradient alone."""
    rw, rb = wgrad_ref.reference(spec['case'])
    sw, sb = rw.abs().max().item() + 1e-30, rb.abs().max().item() + 1e-30
    if spec['accumulate']:
        rw, rb = rw + spec['dw'].double(), rb + spec['db'].double()
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
    ap.add_argument('--cases', type=int, default=200)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--emu', action='store_true', help='run on the host replay (no GPU needed)')
    args = ap.parse_args()
    rng = random.Random(args.seed)
    backend = emulator() if args.emu else device()
    bad = 0
    for i in range(args.cases):
        cfg, msg = one_case(rng, backend, i + 7919 * args.seed)
        if msg:
            bad += 1
            print(f'FAIL case {i}: {msg}\n     {cfg}', flush=True)
    print(f'{args.cases - bad}/{args.cases} tiled head / tail weight gradients within {TOL:g} of float64 '
          f'({"host replay" if args.emu else "device"})')
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
