"""GPU: the single-round-trip 1-D convolution (csrc/conv_small1d.hip) at the C ABI, every instance -- conv_small1d_kernel<16 | 32 | 64>
-- against the float64 reference of tests/small1d_ref.py, on the launches of tests/small1d_cases.py.

Every launch is built through engine.launch_conv and asserts, before any number is looked at, that sda_conv_igemm_path gives 3 and
sda_small1d_tile the tile the case names (tests/test_small1d_host.py proves the same table on the CPU; here the compiled planner of the
machine is asked, so a planner change cannot silently move a case to another instance or to the staged kernel).  The output is
pre-filled with NaN inside a buffer of sentinels: afterwards every element is finite and both guard bands are untouched.

  t64_multi   342 x 97: two 64-position tiles, the last holds 33 positions (fragment 2 partial, fragment 3 empty)
  t64_short   1025 sequences of 1 / 2 / 3 / 5 / 16 positions: shorter than the tile and than the halo; with one position the circular
              neighbours are the position itself
  t32         513 x 32 (a full tile), 600 x 20 (a partial one)
  t16_edge    512 x 32: n * ceil(wo / 16) is exactly 1024, the last shape of the 16-position instance
  t64_cap     4096 x 64: 4096 workgroups, the last grid served; 4097 x 64: declined (path 0, the staged kernel), numbers still right
  channels    (cin, cout) = (64, 64), (17, 33), (3, 64), (64, 1), (40, 16): ragged K quads, waves 1..3 off, cout_pad 16 / 32 / 48 / 64
              (PackedConv pads cout to 32 or 64; the `tight` cases re-pack to cin_pad % 4 == 0 / cout_pad % 16 == 0, the narrowest the kernel takes)
  fusions     per tile: all off, each alone (shared / per-image modulation, LayerNorm, SiLU / ELU loader, bias, SiLU' / ELU' epilogue,
              residual), all on; `all_image_elu` takes every out-of-line branch at once
  views       per tile: channel-last storage (x_sc = 1, x_sx = C), a window view (n_inner > 1), and one launch split in two with
              x_n_off > 0, whose halves equal the whole bit for bit
  backward    the transposed packing of a Conv1d on every tile, against autograd in float64

Tolerance (tests/util.assert_close, scale-relative): the yardstick of a case is the error the float32 evaluation of the same steps on
the CPU (small1d_ref in float32) makes against float64, computed in the test; the bound is 4 x that, never below 2e-6 and never above
1e-4.  Measured max |err| / max |ref| per family, worst case of the family (MI355X), beside the worst yardstick:

  family      cases  device    yardstick
  t64_multi   22     6.51e-07  2.82e-07
  t64_short   13     3.96e-07  2.67e-07
  t32         24     5.74e-07  2.50e-07
  t16_edge    21     5.02e-07  2.64e-07
  t64_cap      4     1.32e-07  1.40e-07
  cross        5     1.61e-07  1.03e-07     (the staged kernel's 1.61e-07; the three tiles 1.375e-07 each)

No yardstick reaches 5e-7, so every case is held at the 2e-6 floor -- 50 times tighter than the 1e-4 of the one older test -- and the
worst device error is a third of it.  No family is ill-conditioned: tests/test_small1d_host.py holds the float32 CPU evaluation of
every case to assert_close's per-element criterion too (no element outside), and every case here uses assert_close whole.  The
3-channel sources run every fusion but the LayerNorm (`all_but_ln`): the statistics of three nearly equal channels would amplify the
float32 rounding of x + mod by up to 1 / sqrt(eps) = 316 for every evaluator.

Cross-tile verdict (n = 4, 40 -> 40 channels, 130 positions, circular, all fusions on; one process per forced SDA_SMALL1D_TP = 16 / 32 /
64): the three outputs are bitwise equal (every instance sums K fragment by K fragment, tap by tap, per 16-position fragment), so
test_three_tiles_agree asserts equality of bits.  The chunked launches agree with it: two 515-image chunks on tile 32 and chunks of
301 and 299 images on tile 16 reproduce their whole launches, on tiles 64 and 32, bit for bit.  The staged kernel (SDA_CONV_SMALL1D=0, path 0) sums in another order and differs from
float64 by 1.61e-07 where the small kernel differs by 1.375e-07; both are held to the same 2e-6.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from sda_amd import _lib, ops
from sda_amd.engine import conv_desc, launch_conv
from tests import small1d_cases as K
from tests import small1d_ref as R
from tests.util import assert_close, rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096                 # floats of sentinel either side of an output
SENTINEL = -12345.0


@pytest.fixture(scope='module')
def dev():
    _lib.load()
    return torch.device('cuda:0')


class Launch:
    """The operands of one case on the device, and its launches."""

    def __init__(self, case, dev):
        self.case, self.dev = case, dev
        self.L = L = R.make_launch(case)
        up = lambda t: None if t is None else t.to(dev).contiguous()
        self.pk = pk = ops.PackedConv(up(L['w_torch']), up(L['b']), transpose=case['transpose'])
        if case['pack'] == 'tight':                          # the same weights at the narrowest padding the kernel takes
            pk.k_pad, pk.m_pad = K.pads(case)
            pk.packed = torch.empty(3 * pk.k_pad * pk.m_pad, device=dev, dtype=torch.float32)
            rows, cols = L['w_torch'].shape[:2]
            ops.pack_conv_weight(up(L['w_torch']), rows, cols, 1, 3, case['transpose'], cols, pk.packed, pk.k_pad, pk.m_pad)
        assert (pk.kh, pk.kw, pk.k_real, pk.m_real) == (1, 3, case['cin'], case['cout'])
        assert (pk.k_pad, pk.m_pad) == K.pads(case)
        self.store = up(L['store'])
        self.mod, self.dact_z, self.res = up(L['mod']), up(L['dact_z']), up(L['res'])
        self.ln = None if L['ln'] is None else (up(L['ln'][0]), up(L['ln'][1]))

    def run(self, lo=0, n=None, path=3, tile=None):
        """Images [lo, lo + n) in one launch -> (out [n][cout][wo], the whole guarded buffer).  `path` / `tile`: what the planner must
        say of the descriptor before the launch."""
        case, L = self.case, self.L
        n = case['n'] if n is None else n
        cout, wo = case['cout'], case['wo']
        numel = n * cout * wo
        buf = torch.full((numel + 2 * GUARD,), SENTINEL, device=self.dev)
        out = buf[GUARD:GUARD + numel].view(n, cout, 1, wo)
        out.fill_(float('nan'))
        rows = slice(lo, lo + n)
        img = lambda t: None if t is None else t[rows].reshape(n, cout, 1, wo)
        src = dict(x_ptr=self.store.data_ptr(), **K.source_fields(case, lo, n))
        opts = dict(circular=case['circular'], bias=self.pk.bias if L['bias'] is not None else None,
                    mod=None if self.mod is None else (self.mod[rows] if L['mod_sn'] else self.mod), mod_sn=L['mod_sn'],
                    ln=None if self.ln is None else (self.ln[0][rows], self.ln[1][rows]), act_in=_lib.ACT_IDS[L['act_in']],
                    dact_z=img(self.dact_z), act_d=_lib.ACT_IDS[L['act_d']], res=img(self.res))
        assert (L['bias'] is None) == (opts['bias'] is None)
        for t in (opts['mod'], opts['dact_z'], opts['res']) + (opts['ln'] or ()):
            assert t is None or t.is_contiguous()
        planned = conv_desc(self.pk, src, out, 1, wo, **opts)
        want_tile = case['tile'] if tile is None else tile
        assert (ops.conv_path(planned) == 3) == (path == 3), f'path {ops.conv_path(planned)}: the launch went to another kernel family'
        assert ops.small1d_tile(planned) == want_tile, 'the planner moved this launch to another tile'
        d = launch_conv(self.pk, src, out, 1, wo, **opts)
        torch.cuda.synchronize()
        assert ops.conv_path(d) == ops.conv_path(planned) and ops.small1d_tile(d) == want_tile
        return out.reshape(n, cout, wo), buf

    def reference(self):
        """float64 [n][cout][wo]; a backward-data case: autograd through the layer itself."""
        case, L = self.case, self.L
        if not case['transpose']:
            return R.small1d_ref(L)
        assert K.FUSIONS[case['fuse']]['mod'] == 'none' and not K.FUSIONS[case['fuse']]['ln'] and L['act_in'] == 'none'
        g = L['store'].reshape(case['n'], case['cin'], case['wo']).double()
        x = torch.zeros(case['n'], case['cout'], case['wo'], dtype=torch.float64, requires_grad=True)
        y = F.conv1d(F.pad(x, (1, 1), mode='circular' if case['circular'] else 'constant'), L['w_torch'].double())
        gx, = torch.autograd.grad(y, x, g)
        if L['dact_z'] is not None:
            gx = gx * R.dact(L['act_d'], L['dact_z'].double())
        if L['res'] is not None:
            gx = gx + L['res'].double()
        return gx


def intact(out, buf, what):
    assert torch.isfinite(out).all(), f'{what}: not every element was written'
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), f'{what}: written outside the output'


def bound(launch, ref64):
    """(yardstick, tolerance) of a case: the float32 CPU evaluation's own error against `ref64`, and 4 x it within [2e-6, 1e-4]."""
    yard = R.yardstick(ref64, R.small1d_ref(launch.L, torch.float32))
    return yard, R.tolerance(yard)


@pytest.mark.parametrize('case', [c for c in K.CASES if c['view'] != 'split'], ids=K.case_id)
def test_launch_matches_float64(dev, case):
    launch = Launch(case, dev)
    out, buf = launch.run(path=3 if case['tile'] else 0)
    intact(out, buf, K.case_id(case))
    ref = launch.reference()
    yard, tol = bound(launch, ref)
    print(f"MEASURED {case['family']} {K.case_id(case)} device={rel_err(out, ref):.3e} yardstick={yard:.3e} tol={tol:.3e}")
    assert_close(out, ref, tol, what=K.case_id(case))


@pytest.mark.parametrize('case', [c for c in K.CASES if c['view'] == 'split'], ids=K.case_id)
def test_chunks_with_an_image_offset_equal_the_whole_launch(dev, case):
    """x_n_off moves the source and nothing else: the chunks, each given its own slice of mod / ln / dact_z / res / out, reproduce
    the whole launch bit for bit (whichever tile each runs on), and the whole launch matches float64."""
    launch = Launch(case, dev)
    whole, buf = launch.run()
    intact(whole, buf, 'whole')
    ref = launch.reference()
    yard, tol = bound(launch, ref)
    print(f"MEASURED {case['family']} {K.case_id(case)} device={rel_err(whole, ref):.3e} yardstick={yard:.3e} tol={tol:.3e}")
    assert_close(whole, ref, tol, what=K.case_id(case))
    for lo, n, tile in case['chunks']:
        part, pbuf = launch.run(lo, n, tile=tile)
        intact(part, pbuf, f'chunk {lo}')
        assert torch.equal(part, whole[lo:lo + n]), f'chunk at image {lo} (tile {tile}) differs from the whole launch (tile {case["tile"]})'


# ------------------------------------------------------------------------------------------ one shape, every tile and both routes

def _child(path, tile):
    """One forced tile or route (both switches are read once per process): the output of CROSS -> an .npy."""
    _lib.load()
    out, buf = Launch(K.CROSS, torch.device('cuda:0')).run(path=3 if tile else 0, tile=tile)
    intact(out, buf, f'child at tile {tile}')
    np.save(path, out.cpu().numpy())


def child_outputs(tmp_path, runs):
    """{name: array} from one fresh process per (name, environment, tile), one after another, each under its own time limit; stops at the
    first that fails."""
    got = {}
    for name, env, tile in runs:
        path = os.path.join(str(tmp_path), f'{name}.npy')
        done = subprocess.run([sys.executable, '-m', 'tests.test_gpu_small1d', path, str(tile)], cwd=ROOT, env=dict(os.environ, **env),
                              timeout=120)
        assert done.returncode == 0, f'the child {name} ended with status {done.returncode}'
        got[name] = np.load(path)
    return got


@pytest.fixture(scope='module')
def cross():
    """(launch operands, float64 reference, tolerance) of CROSS, shared by the two child-process tests."""
    L = R.make_launch(K.CROSS)
    ref = R.small1d_ref(L)
    yard = R.yardstick(ref, R.small1d_ref(L, torch.float32))
    return ref, yard, R.tolerance(yard)


def test_three_tiles_agree(dev, cross, tmp_path):
    """The same launch on the 16-, 32- and 64-position instances (SDA_SMALL1D_TP, one fresh process each): each against float64, and
    bitwise equal to each other -- every instance sums K fragment by K fragment, tap by tap, per 16-position fragment."""
    ref, yard, tol = cross
    got = child_outputs(tmp_path, [(f'tp{tp}', dict(SDA_SMALL1D_TP=str(tp)), tp) for tp in (16, 32, 64)])
    for name, out in got.items():
        print(f'MEASURED cross {name} device={rel_err(torch.from_numpy(out), ref):.3e} yardstick={yard:.3e} tol={tol:.3e}')
        assert_close(torch.from_numpy(out), ref, tol, what=f'{name} vs float64')
    for name in ('tp32', 'tp64'):
        diff = np.abs(got[name].astype(np.float64) - got['tp16']).max()
        assert np.array_equal(got[name], got['tp16']), f'{name} differs from tp16 by up to {diff:.3e}'


def test_staged_kernel_and_small_kernel_agree_with_float64(dev, cross, tmp_path):
    """SDA_CONV_SMALL1D=0 (a fresh process) sends the same launch to the staged kernel of conv_igemm.hip, path 0: both routes are held
    to float64 at the same tolerance (they sum in different orders: no bitwise claim)."""
    ref, yard, tol = cross
    staged = child_outputs(tmp_path, [('staged', dict(SDA_CONV_SMALL1D='0'), 0)])['staged']
    here, buf = Launch(K.CROSS, dev).run()
    intact(here, buf, 'small kernel')
    print(f'MEASURED cross staged device={rel_err(torch.from_numpy(staged), ref):.3e} yardstick={yard:.3e} tol={tol:.3e}')
    print(f'MEASURED cross small1d device={rel_err(here, ref):.3e} yardstick={yard:.3e} tol={tol:.3e}')
    assert_close(torch.from_numpy(staged), ref, tol, what='staged kernel vs float64')
    assert_close(here, ref, tol, what='small kernel vs float64')


if __name__ == '__main__':
    _child(sys.argv[1], int(sys.argv[2]))
