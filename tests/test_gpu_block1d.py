"""GPU: the one-launch residual block of the 1-D nets (csrc/block1d.hip) at the C ABI, every tile instance -- block1d_fwd_kernel /
block1d_bwd_kernel <16 | 32 | 64> -- against the float64 reference of tests/block1d_ref.py: y, z, mean, rstd and gx.

Every case asserts its tile through sda_block1d_tile first (a planner change cannot silently move it back to the 16-position kernels),
pre-fills all five outputs with NaN and requires them finite afterwards.  The shapes are the smallest that reach each path:

  t64_multi   342 x 97: two 64-position tiles, the last holds 33 positions; c = 64 / 33 / 5 (waves 1..3 off, ragged channel groups);
              the second loader pass (columns 64..81), its two statistics registers and the fifth conv1 fragment
  t64_short   1025 sequences of 1 / 2 / 3 / 5 / 16 positions, c = 17: shorter than the tile and than the halo; circular columns wrap twice
  t64_short_c2  the same at c = 2, the narrowest net the kernels take
  t32         513 x 32 (one full tile) and 600 x 20 (a partial one); ELU runs the out-of-line activation switch
  t16_edge    512 x 32: n * ceil(len / 16) is exactly 1024, the last shape of the 16-position kernels

Tolerance (scale-relative: max |err| <= tol * max |ref|): the 16-position kernels, forced with SDA_BLOCK1D_TP=16 on the same inputs,
were measured against float64 per family and output; a case asserts 4 x that figure, never above 1e-4 and never below 2e-6 (fp32
round-off).  Measured max |err| / max |ref| of the 16-position kernels (MI355X):

  family      y         z         mean      rstd      gx
  t64_multi   4.08e-07  5.96e-07  1.43e-07  2.88e-07  4.11e-07
  t64_short   2.32e-07  3.83e-07  1.32e-07  1.08e-07  2.80e-07
  t64_short_c2  3.25e-06  1.82e-05  8.77e-08  8.24e-06  4.84e-05
  t32         3.80e-07  6.36e-07  1.30e-07  1.91e-07  5.91e-07
  t16_edge    4.15e-07  6.20e-07  1.08e-07  1.16e-07  4.06e-07
  cross       2.26e-07  4.19e-07  1.05e-07  1.02e-07  2.64e-07

On the natural tiles (64 / 64 / 64 / 32 / 16) every case gave the same figures to the last digit: the tile only changes which workgroup owns
a column, not the order of any sum.

Every family but t64_short_c2 is asserted with tests/util.assert_close, whose first criterion is the bound above and whose second, per
element (|err| <= tol |ref| + max(tol / 10, 2e-6) max |ref|), is the stricter one above tol = 2e-6.  t64_short_c2 is held to the
scale-relative bound alone: a LayerNorm over two channels that nearly agree is ill-conditioned in fp32 whoever computes it -- the mean
carries a rounding of 2^-24 |mean|, the centred values are differences of that size over sqrt(var + eps) >= 3.2e-3, so xh is off by up to
2e-5 |mean| -- and elements of z with a small reference value then miss the per-element criterion on every tile, the 16-position one
included (the outputs are bitwise the same): at tol = 7.3e-5, 2 of 32800 at 1025 x 16, |err| = 1.0e-5 where |ref| = 1.5e-2, max |ref| = 0.82.

Cross-tile verdict (n = 4, c = 40, len = 130, circular, SiLU; one process per forced tile): all five outputs of the three
tiles are bitwise equal, so the test asserts equality of bits.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from sda_amd import _lib, ops
from tests import block1d_ref as R
from tests.util import assert_close, rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ('y', 'z', 'mean', 'rstd', 'gx')
EPS = 1e-5

# max |err| / max |ref| of the 16-position kernels per family and output (see the module docstring)
MEASURED_TP16 = {
    't64_multi': dict(y=4.083e-07, z=5.957e-07, mean=1.434e-07, rstd=2.880e-07, gx=4.108e-07),
    't64_short': dict(y=2.320e-07, z=3.829e-07, mean=1.319e-07, rstd=1.077e-07, gx=2.804e-07),
    't64_short_c2': dict(y=3.245e-06, z=1.817e-05, mean=8.772e-08, rstd=8.237e-06, gx=4.839e-05),
    't32': dict(y=3.795e-07, z=6.356e-07, mean=1.296e-07, rstd=1.913e-07, gx=5.914e-07),
    't16_edge': dict(y=4.149e-07, z=6.196e-07, mean=1.081e-07, rstd=1.157e-07, gx=4.062e-07),
    'cross': dict(y=2.258e-07, z=4.187e-07, mean=1.051e-07, rstd=1.019e-07, gx=2.643e-07),
}


def tolerance(family, name):
    return min(max(4.0 * MEASURED_TP16[family][name], 2e-6), 1e-4)


def check(out, ref, family, name, what):
    """`out` against float64 at the family's tolerance (see the module docstring for the one family without the per-element criterion)."""
    tol = tolerance(family, name)
    if family == 't64_short_c2':
        assert out.shape == ref.shape, what
        err = rel_err(out, ref)
        assert err <= tol, f'{what}: max |err| / max |ref| = {err:.3e} > {tol:.3e}'
    else:
        assert_close(out, ref, tol, what=what)


def _case(family, tile, n, length, c, padding, act='SiLU', mod='sample', unbiased=True):
    return dict(family=family, tile=tile, n=n, len=length, c=c, circular=padding == 'circular', act=act, mod=mod, unbiased=unbiased)


def _id(k):
    return (f"{k['family']}-n{k['n']}-len{k['len']}-c{k['c']}-{'circular' if k['circular'] else 'zeros'}-{k['act']}-mod_{k['mod']}-"
            f"{'unbiased' if k['unbiased'] else 'biased'}")


CASES = (
    # tile 64, several tiles, partial last tile (per-sample modulation)
    [_case('t64_multi', 64, 342, 97, c, p) for c in (64, 33, 5) for p in ('zeros', 'circular')] +
    [_case('t64_multi', 64, 342, 97, 33, 'circular', unbiased=False),
     _case('t64_multi', 64, 342, 97, 5, 'zeros', act='ELU')] +
    # tile 64, sequence shorter than the tile and than the halo (shared modulation and none)
    [_case('t64_short' if c == 17 else 't64_short_c2', 64, 1025, L, c, p, mod=m)
     for L in (1, 2, 3, 5, 16) for c in (2, 17) for p in ('circular', 'zeros') for m in ('shared', 'none')] +
    [_case('t64_short', 64, 1025, 3, 17, 'circular', mod='shared', unbiased=False)] +
    # tile 32
    [_case('t32', 32, n, L, c, p, act=a) for n, L in ((513, 32), (600, 20)) for c in (64, 6) for p in ('zeros', 'circular')
     for a in (('SiLU', 'ELU') if (n, c) in ((513, 6), (600, 64)) else ('SiLU',))] +
    [_case('t32', 32, 600, 20, 6, 'circular', unbiased=False)] +
    # tile 16 at the boundary
    [_case('t16_edge', 16, 512, 32, 48, 'circular'), _case('t16_edge', 16, 512, 32, 48, 'circular', unbiased=False)]
)
CROSS = _case('cross', None, 4, 130, 40, 'circular')

# one case per tile for the save-less forward and the run-to-run checks
PER_TILE = [_case('t64_multi', 64, 342, 97, 33, 'circular'), _case('t64_short', 64, 1025, 3, 17, 'circular', mod='shared'),
            _case('t32', 32, 600, 20, 6, 'zeros', act='ELU'), _case('t16_edge', 16, 512, 32, 48, 'circular')]


@pytest.fixture(scope='module')
def dev():
    _lib.load()
    return torch.device('cuda:0')


class Block:
    """One random block at the C ABI: torch-layout weights, their forward / backward-data packings, input, modulation, cotangent."""

    def __init__(self, k, dev):
        seed = (k['n'] * 1009 + k['len'] * 131 + k['c'] * 7 + int(k['circular'])) % (2 ** 31)
        g = torch.Generator().manual_seed(seed)
        n, c, L = k['n'], k['c'], k['len']
        rnd = lambda *s: torch.randn(*s, generator=g)
        self.k, self.dev = k, dev
        self.w1, self.w2 = (rnd(c, c, 3) / (3 * c) ** 0.5).to(dev), (rnd(c, c, 3) / (3 * c) ** 0.5).to(dev)
        self.b1, self.b2 = (0.1 * rnd(c)).to(dev), (0.1 * rnd(c)).to(dev)
        self.a = rnd(n, c, 1, L).to(dev)
        self.g = rnd(n, c, 1, L).to(dev)
        rows = dict(sample=n, shared=1, none=0)[k['mod']]
        self.mod = (0.5 * rnd(rows, c)).to(dev) if rows else None
        self.mod_sn = c if rows == n else 0
        self.pk1, self.pk2 = ops.PackedConv(self.w1, self.b1), ops.PackedConv(self.w2, self.b2)
        self.pk1b, self.pk2b = ops.PackedConv(self.w1, None, transpose=True), ops.PackedConv(self.w2, None, transpose=True)
        assert ops.block1d_eligible(c, 1, self.pk1, self.pk2)
        self.act = _lib.ACT_IDS[k['act']]

    def tile(self):
        k = self.k
        return ops.block1d_tile(ops._block1d_desc(self.a, self.mod, self.mod_sn, self.pk1, self.pk2, k['circular'], self.act, EPS,
                                                  k['unbiased']))

    def run(self, save=True):
        """-> dict of the outputs (gx only with the saves), each pre-filled with NaN."""
        k = self.k
        n, c, L = k['n'], k['c'], k['len']
        nan = lambda *s: torch.full(s, float('nan'), device=self.dev)
        out = dict(y=nan(n, c, 1, L))
        if save:
            out.update(z=nan(n, c, 1, L), mean=nan(n * L), rstd=nan(n * L), gx=nan(n, c, 1, L))
        ops.block1d_fwd(self.a, self.mod, self.mod_sn, self.pk1, self.pk2, k['circular'], self.act, EPS, k['unbiased'], out['y'],
                        out.get('z'), out.get('mean'), out.get('rstd'))
        if save:
            ops.block1d_bwd(self.g, self.a, out['z'], out['mean'], out['rstd'], self.mod, self.mod_sn, self.pk1b, self.pk2b,
                            k['circular'], self.act, k['unbiased'], out['gx'])
        torch.cuda.synchronize()
        shape = dict(y=(n, c, L), z=(n, c, L), gx=(n, c, L), mean=(n, L), rstd=(n, L))
        return {name: t.reshape(shape[name]) for name, t in out.items()}

    def reference(self):
        k = self.k
        sq = lambda t: t.reshape(k['n'], k['c'], k['len'])
        return R.block1d_reference(sq(self.a), self.mod, self.w1, self.b1, self.w2, self.b2, sq(self.g), k['circular'], k['act'], EPS,
                                   k['unbiased'])


def errors(k, dev):
    """{output: max |err| / max |ref|} of one case on whichever tile the process runs (the measurement behind MEASURED_TP16)."""
    blk = Block(k, dev)
    out, ref = blk.run(), blk.reference()
    return {name: rel_err(out[name], ref[name]) for name in OUTPUTS}


@pytest.mark.parametrize('k', CASES, ids=_id)
def test_block_matches_float64(dev, k):
    blk = Block(k, dev)
    assert blk.tile() == k['tile'], 'the planner moved this case to another tile'
    out, ref = blk.run(), blk.reference()
    for name in OUTPUTS:
        assert torch.isfinite(out[name]).all(), f'{name}: not every element was written'
    errs = {name: rel_err(out[name], ref[name]) for name in OUTPUTS}
    print(_id(k), ' '.join(f'{name}={e:.2e}' for name, e in errs.items()))
    for name in OUTPUTS:
        check(out[name], ref[name], k['family'], name, f'{name} vs float64')


@pytest.mark.parametrize('k', PER_TILE, ids=_id)
def test_saveless_forward_and_rerun_are_bitwise_equal(dev, k):
    """The forward that keeps nothing for the VJP (z / mean / rstd NULL) writes the same y; a second run of forward and VJP gives the
    same bits (fixed-order reductions, no atomics)."""
    blk = Block(k, dev)
    assert blk.tile() == k['tile'], 'the planner moved this case to another tile'
    first, again, bare = blk.run(), blk.run(), blk.run(save=False)
    assert torch.isfinite(bare['y']).all()
    assert torch.equal(bare['y'], first['y'])
    for name in OUTPUTS:
        assert torch.equal(first[name], again[name]), name


def test_two_level_net_runs_on_the_64_position_kernels(dev, monkeypatch):
    """A two-level 1-D U-Net at a batch whose every block runs on the 64-position kernels: forward and input VJP through the engine
    against the float64 oracle."""
    import torch.nn as nn
    from oracle import sda_oracle as O
    from sda_amd.nn import UNet
    torch.manual_seed(11)
    channels, hidden, length, batch = 3, (16, 32), 32, 1100
    net = UNet(channels, channels, 16, hidden_channels=hidden, hidden_blocks=(1, 1), kernel_size=3, activation=nn.SiLU, spatial=1,
               padding_mode='circular').to(dev)
    x = torch.randn(batch, channels, length, device=dev)
    emb = torch.randn(batch, 16, device=dev)
    g = torch.randn(batch, channels, length, device=dev)
    tiles = dict(fwd=[], bwd=[])
    real_fwd, real_bwd = ops.block1d_fwd, ops.block1d_bwd

    def fwd(a, mod, mod_sn, pk1, pk2, circular, act, eps, unbiased, *rest):
        tiles['fwd'].append((a.shape[1], ops.block1d_tile(ops._block1d_desc(a, mod, mod_sn, pk1, pk2, circular, act, eps, unbiased))))
        return real_fwd(a, mod, mod_sn, pk1, pk2, circular, act, eps, unbiased, *rest)

    def bwd(g_, a, z, mean, rstd, mod, mod_sn, pk1b, pk2b, circular, act, unbiased, gx):
        tiles['bwd'].append((a.shape[1], ops.block1d_tile(ops._block1d_desc(a, mod, mod_sn, pk1b, pk2b, circular, act, 0.0, unbiased))))
        return real_bwd(g_, a, z, mean, rstd, mod, mod_sn, pk1b, pk2b, circular, act, unbiased, gx)

    assert ops.BLOCK1D
    monkeypatch.setattr(ops, 'block1d_fwd', fwd)
    monkeypatch.setattr(ops, 'block1d_bwd', bwd)
    xx = x.clone().requires_grad_(True)
    y = net(xx, emb)
    gx, = torch.autograd.grad(y, xx, g)
    # a descent and an ascent block per level (16 channels x 32 positions, 32 channels x 16 positions), forward and backward
    for way in ('fwd', 'bwd'):
        assert sorted(tiles[way]) == [(16, 64), (16, 64), (32, 64), (32, 64)], (way, tiles[way])
    sd = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    cfg = O.UNetConfig(channels, channels, 16, hidden, (1, 1), 3, 2, 'SiLU', 1, 'circular')
    xo = x.cpu().double().requires_grad_(True)
    yo = O.unet_forward(sd, '', cfg, xo, emb.cpu().double())
    gxo, = torch.autograd.grad(yo, xo, g.cpu().double())
    assert_close(y.detach(), yo.detach().float(), 1e-4, what='forward vs oracle')
    assert_close(gx, gxo.float(), 1e-4, what='VJP vs oracle')


def _child(path):
    """One forced tile (SDA_BLOCK1D_TP is read once per process): the five outputs of CROSS -> an .npz."""
    _lib.load()
    out = Block(CROSS, torch.device('cuda:0')).run()
    np.savez(path, **{name: t.cpu().numpy() for name, t in out.items()})


def cross_tile_outputs(tmp_path):
    """{tile: {output: array}} from one fresh process per forced tile, one after another; stops at the first that fails."""
    got = {}
    for tp in (16, 32, 64):
        path = os.path.join(str(tmp_path), f'tp{tp}.npz')
        env = dict(os.environ, SDA_BLOCK1D_TP=str(tp))
        done = subprocess.run([sys.executable, '-m', 'tests.test_gpu_block1d', path], cwd=ROOT, env=env, timeout=120)
        assert done.returncode == 0, f'the child forced to tile {tp} ended with status {done.returncode}'
        with np.load(path) as f:
            got[tp] = {name: f[name] for name in OUTPUTS}
    return got


def test_three_tiles_agree(dev, tmp_path):
    """The same block on the 16-, 32- and 64-position kernels (SDA_BLOCK1D_TP, one fresh process each): each against float64, and
    bitwise equal to each other -- the tile decides which workgroup owns a column, never the order of a sum."""
    got = cross_tile_outputs(tmp_path)
    ref = Block(CROSS, dev).reference()
    for tp, out in got.items():
        for name in OUTPUTS:
            assert np.isfinite(out[name]).all(), f'tile {tp}, {name}: not every element was written'
            check(torch.from_numpy(out[name]), ref[name], 'cross', name, f'tile {tp}, {name} vs float64')
    for tp in (32, 64):
        for name in OUTPUTS:
            assert np.array_equal(got[tp][name], got[16][name]), f'{name}: tile {tp} differs from tile 16'


if __name__ == '__main__':
    _child(sys.argv[1])
