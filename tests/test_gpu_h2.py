"""GPU: the OPT-IN f16 x 2 multiply (csrc/conv_h2.hip; ops.set_multiply('f16x2') / SDA_MULTIPLY / bench.py --multiply f16x2).

Every fp32 operand of the block convolutions (sda/nn.py:131-142 and their backward-data) is split into two halves, hi + lo, and the
multiply runs as three f16 MFMA products with fp32 accumulation.  Checked here:
  (i)   single launches -- every loader / epilogue the reference's blocks use, forward and backward-data packings, both padding modes,
        input magnitudes from 1e-3 to 1e3 -- against a float64 convolution: <= 3e-6 of the output's scale (the fp32 kernels: <= 2e-6);
  (ii)  the reference's Kolmogorov net at 64 x 64: score, guided score and input VJP against the oracle at the suite's rtol 1e-4,
        and against the SAME evaluation on the fp32 kernels;
  (iii) 16 free-running guided predictor-corrector steps through the hipGraph against the fp32 oracle at rtol 1e-4;
  (iv)  the launch reports max |out| exactly, and shapes the kernel does not serve fall back to the fp32 kernels."""
import math

import os

import pytest
import torch
import torch.nn.functional as F

from oracle import sda_oracle as O
from tests.util import assert_close, oracle_eps_from_module, rel_err

pytestmark = pytest.mark.gpu
K64 = dict(window=5, embedding=64, hidden_channels=(96, 192, 384), hidden_blocks=(3, 3, 3))


@pytest.fixture(scope='module')
def dev():
    from sda_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


@pytest.fixture
def f16x2():
    from sda_amd import ops
    prev = ops.set_multiply('f16x2')
    yield
    ops.set_multiply(prev)


def _ref64(x, w, bias, circular, transpose, ln, mod, silu_in, dact_z, res):
    x, w = x.double().cpu(), w.double().cpu()
    if ln:
        u = x + (0 if mod is None else mod.double().cpu().reshape(1, -1, 1, 1))
        var, mean = torch.var_mean(u, dim=1, unbiased=True, keepdim=True)
        x = (u - mean) / torch.sqrt(var + 1e-5)
    if silu_in:
        x = F.silu(x)
    xp = F.pad(x, (1, 1, 1, 1), mode='circular') if circular else F.pad(x, (1, 1, 1, 1))
    if transpose:
        w = w.flip(2, 3).transpose(0, 1)
    y = F.conv2d(xp, w, None if bias is None else bias.double().cpu())
    if dact_z is not None:
        z = dact_z.double().cpu()
        s = torch.sigmoid(z)
        y = y * (s * (1 + z * (1 - s)))
    if res is not None:
        y = y + res.double().cpu()
    return y


CASES = [('plain', {}), ('mod+LN', dict(ln=True, mod=True)), ('LN', dict(ln=True)), ('SiLU+res', dict(silu=True, res=True)), ('dact', dict(dact=True))]


@pytest.mark.parametrize('cin,cout,hw,n', [(96, 96, 32, 2), (192, 96, 16, 3), (96, 192, 48, 1), (384, 384, 16, 2),
                                           # round 6: the 64-cout tile and K % 32 (the reference's default widths (64, 128, 256), mixed with 96-multiples)
                                           (64, 64, 32, 2), (128, 256, 16, 3), (256, 128, 32, 1), (96, 64, 16, 2), (320, 64, 16, 1)])
@pytest.mark.parametrize('transpose', [False, True])
def test_h2_launches_vs_float64(dev, f16x2, cin, cout, hw, n, transpose):
    from sda_amd import ops
    from sda_amd.engine import launch_conv, planar_source
    torch.manual_seed(cin + cout + hw + int(transpose))
    for circular in (True, False):
        for name, fz in CASES:
            scale = 10.0 ** torch.randint(-3, 4, (1,)).item()
            x = torch.randn(n, cout if transpose else cin, hw, hw, device=dev) * scale
            w = (torch.rand(cout, cin, 3, 3, device=dev) * 2 - 1) / math.sqrt(cin * 9)
            b = None if transpose else torch.randn(cout, device=dev)
            pk = ops.PackedConv(w, b, transpose=transpose)
            assert pk.h2 is not None
            out = torch.empty(n, cin if transpose else cout, hw, hw, device=dev)
            mod = torch.randn(x.shape[1], device=dev) * scale if fz.get('mod') else None
            ln = None
            if fz.get('ln'):
                u = x + (0 if mod is None else mod.reshape(1, -1, 1, 1))
                var, mean = torch.var_mean(u, dim=1, unbiased=True)
                ln = (mean.reshape(-1).contiguous(), (1 / torch.sqrt(var + 1e-5)).reshape(-1).contiguous())
            dz = torch.randn_like(out) if fz.get('dact') else None
            rs = torch.randn_like(out) * scale if fz.get('res') else None
            kw = dict(circular=circular, bias=pk.bias, act_in=1 if fz.get('silu') else 0, res=rs)
            if ln is not None:
                kw['ln'] = ln
                if mod is not None:
                    kw.update(mod=mod, mod_sn=0)
            if dz is not None:
                kw.update(dact_z=dz, act_d=1)
            xa = None if ln is not None else ops.absmax(x, pk.in_amax)
            d = launch_conv(pk, planar_source(x), out, hw, hw, x_amax=xa, out_amax=pk.out_amax, **kw)
            assert d.w_h2, f'{name}: the f16 x 2 kernel did not serve the launch'
            ref = _ref64(x, w, b, circular, transpose, ln is not None, mod, fz.get('silu'), dz, rs)
            err = ((out.double().cpu() - ref).abs().max() / ref.abs().max()).item()
            assert err <= 3e-6, f'{cin}->{cout} @{hw} {"bwd" if transpose else "fwd"} {"circ" if circular else "zero"} {name} x~{scale:g}: {err:.2e}'
            assert abs(pk.out_amax.item() - out.abs().max().item()) <= 1e-6 * out.abs().max().item()


def test_h2_scale_and_fallbacks(dev, f16x2):
    from sda_amd import _lib, ops
    from sda_amd.engine import launch_conv, planar_source
    lib = _lib.load()
    for amax, want in ((1.0, 1024.0), (1.5, 1024.0), (2.0, 512.0), (1000.0, 2.0), (3e-3, 2.0 ** 19), (0.0, 1.0), (float('inf'), 1.0)):
        assert lib.sda_conv_h2_scale(amax) == want, (amax, lib.sda_conv_h2_scale(amax))
    assert lib.sda_conv_h2_packed_bytes(96, 96, 0) == 6 * 9 * 6 * 1024 and lib.sda_conv_h2_packed_bytes(96, 11, 0) == 0
    assert lib.sda_conv_h2_packed_bytes(64, 64, 0) == 4 * 9 * 4 * 1024 and lib.sda_conv_h2_packed_bytes(32, 64, 0) == 0 and lib.sda_conv_h2_packed_bytes(64, 48, 0) == 0
    # a 3 x 3 layer whose channels do not tile (11 -> 96, the head) and an image that does not tile by 16: the fp32 kernels serve them
    for cin, cout, hw in ((11, 96, 32), (96, 96, 24)):
        x = torch.randn(1, cin, hw, hw, device=dev)
        w = torch.randn(cout, cin, 3, 3, device=dev) * 0.05
        pk = ops.PackedConv(w, None)
        out = torch.empty(1, cout, hw, hw, device=dev)
        d = launch_conv(pk, planar_source(x), out, hw, hw, circular=True, x_amax=None if pk.h2 is None else ops.absmax(x, pk.in_amax))
        assert not d.w_h2
        ref = F.conv2d(F.pad(x.double().cpu(), (1, 1, 1, 1), mode='circular'), w.double().cpu())
        assert rel_err(out, ref) < 2e-6
    # without a magnitude for the input the launch stays on the fp32 kernels, too
    x = torch.randn(1, 96, 32, 32, device=dev)
    pk = ops.PackedConv(torch.randn(96, 96, 3, 3, device=dev) * 0.05, None)
    d = launch_conv(pk, planar_source(x), torch.empty_like(x), 32, 32, circular=True)
    assert pk.h2 is not None and not d.w_h2


@pytest.fixture(scope='module')
def k64(dev):
    from sda_amd.experiments.kolmogorov import make_score
    torch.manual_seed(90)
    net = make_score(size=64, **K64)
    return net, oracle_eps_from_module(net, 'mc2d')


def test_h2_k64_score_guided_and_vjp_vs_oracle(dev, k64):
    _score_guided_and_vjp_check(dev, *k64, length=6, label='K64')


def test_h2_default_width_net_score_guided_and_vjp_vs_oracle(dev):
    """Round 6: the opt-in route on the reference's DEFAULT widths -- `make_score()` as experiments/kolmogorov/utils.py:49-57 builds it
    (window 3, (64, 128, 256)): conv_h2's 64-cout tile (MB = 2), contractions of 64 / 128 / 256 channels (K % 32; the ring across tiles)."""
    from sda_amd.experiments.kolmogorov import make_score
    torch.manual_seed(95)
    net = make_score(size=64)
    _score_guided_and_vjp_check(dev, net, oracle_eps_from_module(net, 'mc2d'), length=4, label='default widths (64, 128, 256)')


def _score_guided_and_vjp_check(dev, net, eps_o, length, label):
    from sda_amd import observe as Ob
    from sda_amd import ops
    from sda_amd.score import GaussianScore, VPSDE
    net.to(dev)
    torch.manual_seed(91)
    x = torch.randn(2, length, 2, 64, 64)
    t = torch.tensor(0.37)
    sub4 = lambda v: v[..., ::4, ::4]
    y = torch.randn(sub4(x).shape)
    g = torch.randn_like(x)
    res = {}
    for mode in ('f32', 'f16x2'):
        prev = ops.set_multiply(mode)
        try:
            launched = []
            real = ops.conv_h2
            ops.conv_h2 = lambda *a, **k: (lambda r: (launched.append(r), r)[1])(real(*a, **k))
            xd = x.to(dev).requires_grad_(True)
            out = net(xd, t.to(dev))
            vjp, = torch.autograd.grad(out, xd, g.to(dev))
            gs = GaussianScore(y, A=Ob.Subsample.space(4), std=0.1, sde=VPSDE(net, shape=())).to(dev)
            guided = gs(x.to(dev), t.to(dev))
            res[mode] = (out.detach().cpu(), vjp.cpu(), guided.cpu(), sum(launched))
        finally:
            ops.conv_h2 = real
            ops.set_multiply(prev)
    assert res['f32'][3] == 0
    assert res['f16x2'][3] >= 2 * 2 * 36, f"only {res['f16x2'][3]} launches took the f16 x 2 kernel"     # 36 block convolutions, fwd + VJP, two evaluations
    ref = eps_o(x, t)
    xo = x.double().requires_grad_(True)
    ref_v, = torch.autograd.grad(eps_o(xo, t.double(), torch.float64), xo, g.double())
    ref_g = O.gaussian_score(eps_o, O.Schedule(), y, sub4, 0.1, 1e-2, x, t)
    for mode in ('f32', 'f16x2'):
        out, vjp, guided, _ = res[mode]
        assert_close(out, ref, 1e-4, what=f'eps ({mode})')
        assert_close(vjp, ref_v, 1e-4, what=f'vjp ({mode})')
        assert_close(guided, ref_g, 1e-4, what=f'guided ({mode})')
    # the two multiplies agree with each other far inside the tolerance
    e = [rel_err(res['f16x2'][i], res['f32'][i].double()) for i in range(3)]
    r32 = [rel_err(res['f32'][0], ref.double()), rel_err(res['f32'][1], ref_v), rel_err(res['f32'][2], ref_g.double())]
    r16 = [rel_err(res['f16x2'][0], ref.double()), rel_err(res['f16x2'][1], ref_v), rel_err(res['f16x2'][2], ref_g.double())]
    print(f'{label} @ 64^2 (eps, vjp, guided): f16x2 vs f32 kernels {e[0]:.1e} {e[1]:.1e} {e[2]:.1e}; vs oracle f32 {r32[0]:.1e} {r32[1]:.1e} {r32[2]:.1e}, '
          f'f16x2 {r16[0]:.1e} {r16[1]:.1e} {r16[2]:.1e}')
    assert max(e) < 2e-5


def test_h2_free_running_guided_hipgraph_vs_fp32_oracle(dev, k64, f16x2):
    import bench
    from sda_amd import observe as Ob
    from sda_amd.parallel import KeyedNoise
    from sda_amd.score import GaussianScore, VPSDE
    net, eps_net = k64
    net.to(dev)
    steps, corr, tau, std, gamma = (16 if os.environ.get('SDA_LONG_TESTS', '0') == '1' else 8), 1, 0.5, 0.1, 1e-2
    event = (6, 2, 64, 64)
    sub4 = lambda v: v[..., ::4, ::4]
    torch.manual_seed(92)
    x1 = torch.randn((1,) + event)
    y = torch.randn(sub4(x1[0]).shape)
    ns = KeyedNoise((0, 1), event, 78, corr, dev)
    zs = torch.stack([ns(i, j) for i in range(steps) for j in range(corr)]).cpu()
    score = bench.SyntheticScore(net)
    inner = VPSDE(score, shape=())
    object.__setattr__(score, '_sched', inner)
    gs = GaussianScore(y, A=Ob.Subsample.space(4), std=std, sde=inner, gamma=gamma)
    sde = VPSDE(gs, shape=event).to(dev)
    sde.initial_noise, sde.noise_source = x1, ns
    sampler = sde.sampler((1,), steps=steps, corrections=corr, tau=tau).capture()
    for _ in range(steps):
        sampler.step()
    got = sampler.result().cpu()
    sched = O.Schedule()

    def eps(xx, tt):
        mu, sg = sched.mu(tt), sched.sigma(tt)
        return xx * (sg / (mu * mu + sg * sg)) + 0.1 * eps_net(xx, tt)
    sc = lambda xx, tt: O.gaussian_score(eps, sched, y, sub4, std, gamma, xx, tt)
    ref32 = O.sample(sc, sched, x1, 4, steps, corr, tau, noise=lambda i, j: zs[i * corr + j])
    err = rel_err(got.double(), ref32.double())
    print(f'f16x2, K64 @ 64^2, {steps} guided PC steps through the hipGraph vs the fp32 oracle: {err:.2e}')
    assert torch.isfinite(got).all() and err <= 1e-4


@pytest.mark.parametrize('c,h,w_,n,pool', [(96, 64, 64, 5, (1, 1)), (192, 64, 96, 3, (1, 1)), (384, 64, 64, 4, (1, 1)), (192, 64, 64, 4, (2, 2)),
                                           (96, 32, 32, 3, (1, 1)), (40, 64, 64, 5, (1, 1)), (96, 6, 5, 1, (1, 1))])
def test_ln_bwd_reports_the_max_of_its_output(dev, c, h, w_, n, pool):
    """sda_ln_bwd_amax (ABI v12): the same gx bit for bit, and amax[0] = max |gx| -- from the kernel's own epilogue on the U-Net levels'
    layouts (>= 16 384 pixels, 49 .. 384 channels), through an absmax pass on the others (few pixels; 40 channels) -- also when the scalar holds a larger stale value."""
    from sda_amd import ops
    torch.manual_seed(c + h)
    x = torch.randn(n, c, h, w_, device=dev) * 3
    mod = torch.randn(n, c, device=dev)
    mean = torch.empty(n * h * w_, device=dev)
    rstd = torch.empty_like(mean)
    ops.ln_stats(x, mod, c, 1e-5, True, mean, rstd)
    gh = torch.randn(n, c, pool[0] * h, pool[1] * w_, device=dev) * 10
    res = torch.randn(n, c, h, w_, device=dev)
    gx0, gx1 = torch.empty_like(x), torch.empty_like(x)
    ops.ln_bwd(gh, x, h, w_, mod, c, mean, rstd, True, pool, res, gx0)
    amax = torch.full((1,), 1e30, device=dev)
    ops.ln_bwd(gh, x, h, w_, mod, c, mean, rstd, True, pool, res, gx1, out_amax=amax)
    assert torch.equal(gx0, gx1)
    assert amax.item() == gx1.abs().max().item()


@pytest.mark.parametrize('cin,cout,hs,ws,n,circular,ln,with_res', [(192, 96, 16, 16, 2, True, True, True), (384, 192, 16, 32, 1, False, True, True),
                                                                   (96, 96, 32, 16, 3, True, False, False), (192, 96, 48, 16, 1, False, True, False),
                                                                   (128, 64, 16, 32, 2, True, True, True), (256, 128, 16, 16, 1, False, True, True)])
def test_h2_upsampled_tail_vs_float64(dev, f16x2, cin, cout, hs, ws, n, circular, ln, with_res):
    """The tails (LayerNorm -> Upsample(nearest, 2) -> conv 3 x 3, sda/nn.py:161-169) on conv_h2's parity-class form (four 2 x 2-tap
    convolutions of the low-resolution tile with pre-summed taps) against float64 and against the zero-position Winograd kernel."""
    from sda_amd import ops
    from sda_amd.engine import launch_conv, planar_source
    torch.manual_seed(cin + hs + ws)
    x = torch.randn(n, cin, hs, ws, device=dev) * 1.7 + 0.3
    w = (torch.rand(cout, cin, 3, 3, device=dev) * 2 - 1) / math.sqrt(cin * 9)
    b = torch.randn(cout, device=dev)
    pk = ops.PackedConv(w, b)
    assert pk.h2 is not None and pk.h2_up() is not None
    out = torch.full((n, cout, 2 * hs, 2 * ws), float('nan'), device=dev)
    res = torch.randn_like(out) if with_res else None
    kw = dict(circular=circular, bias=pk.bias, up=(2, 2), res=res)
    x64 = x.double().cpu()
    if ln:
        var, mean = torch.var_mean(x, dim=1, unbiased=True)
        kw['ln'] = (mean.reshape(-1).contiguous(), (1 / torch.sqrt(var + 1e-5)).reshape(-1).contiguous())
        v64, m64 = torch.var_mean(x64, dim=1, unbiased=True, keepdim=True)
        x64 = (x64 - m64) / torch.sqrt(v64 + 1e-5)
    xu = x64.repeat_interleave(2, -1).repeat_interleave(2, -2)
    xp = F.pad(xu, (1, 1, 1, 1), mode='circular') if circular else F.pad(xu, (1, 1, 1, 1))
    ref = F.conv2d(xp, w.double().cpu(), b.double().cpu())
    if res is not None:
        ref = ref + res.double().cpu()
    d = launch_conv(pk, planar_source(x), out, 2 * hs, 2 * ws, x_amax=None if ln else ops.absmax(x, pk.in_amax), **kw)
    assert d.w_h2 and d.up_h == 2, 'the up-sampled launch was not served by conv_h2'
    err = ((out.double().cpu() - ref).abs().max() / ref.abs().max()).item()
    prev, ops.H2_UP = ops.H2_UP, False
    try:
        out32 = torch.empty_like(out)
        d32 = launch_conv(pk, planar_source(x), out32, 2 * hs, 2 * ws, x_amax=None if ln else ops.absmax(x, pk.in_amax), **kw)
        assert not d32.w_h2
    finally:
        ops.H2_UP = prev
    err32 = ((out32.double().cpu() - ref).abs().max() / ref.abs().max()).item()
    print(f'up-sampled tail {cin}->{cout} @{hs}x{ws}: f16x2 parity-class form {err:.2e}, zero-position Winograd {err32:.2e} (vs float64, of max |ref|)')
    assert err < 3e-6


@pytest.mark.parametrize('cin,cout,hs,ws,n,circular', [(192, 96, 16, 16, 2, True), (384, 192, 16, 32, 1, False), (96, 96, 32, 16, 3, True),
                                                       (192, 96, 48, 16, 1, False), (128, 64, 16, 32, 2, True), (256, 128, 16, 16, 1, False)])
def test_h2_pooled_tail_vjp_vs_float64_autograd(dev, f16x2, cin, cout, hs, ws, n, circular):
    """The VJP of Upsample(nearest, 2) -> conv 3 x 3 (the tails' backward, sda/score.py:394 through sda/nn.py:161-169) on conv_h2's
    parity-plane form (a 2 x 2-tap convolution over the four parity planes of the fine-resolution gradient, K = 4 x cout) against
    float64 autograd through the up-sample and against the zero-position Winograd kernel's pooled launch."""
    from sda_amd import ops
    from sda_amd.engine import launch_conv, planar_source
    torch.manual_seed(cin + hs + 3 * ws)
    w = (torch.rand(cout, cin, 3, 3, device=dev) * 2 - 1) / math.sqrt(cin * 9)
    pk = ops.PackedConv(w, None, transpose=True)
    assert pk.h2 is not None and pk.h2_pool() is not None
    g = torch.randn(n, cout, 2 * hs, 2 * ws, device=dev) * 0.7
    x64 = torch.zeros(n, cin, hs, ws, dtype=torch.float64, requires_grad=True)
    xu = x64.repeat_interleave(2, -1).repeat_interleave(2, -2)
    xp = F.pad(xu, (1, 1, 1, 1), mode='circular') if circular else F.pad(xu, (1, 1, 1, 1))
    ref, = torch.autograd.grad(F.conv2d(xp, w.double().cpu()), x64, g.double().cpu())
    out = torch.full((n, cin, hs, ws), float('nan'), device=dev)
    d = launch_conv(pk, planar_source(g), out, 2 * hs, 2 * ws, circular=circular, pool=(2, 2), x_amax=ops.absmax(g, pk.in_amax))
    assert d is not None and d.w_h2 and d.pool_h == 2, 'the pooled launch was not served by conv_h2'
    err = ((out.double().cpu() - ref).abs().max() / ref.abs().max()).item()
    out32 = torch.empty_like(out)
    d32 = launch_conv(pk, planar_source(g), out32, 2 * hs, 2 * ws, circular=circular, pool=(2, 2))
    assert d32 is not None and not d32.w_h2
    err32 = ((out32.double().cpu() - ref).abs().max() / ref.abs().max()).item()
    print(f'pooled tail VJP {cout}->{cin} @{hs}x{ws}: f16x2 parity-plane form {err:.2e}, zero-position Winograd {err32:.2e} (vs float64 autograd, of max |ref|)')
    assert err < 3e-6


@pytest.mark.parametrize('cin,cout,hs,ws,n,circular', [(96, 192, 32, 32, 2, True), (192, 384, 32, 64, 1, False), (96, 96, 64, 32, 3, True),
                                                       (96, 192, 96, 32, 1, False), (64, 128, 32, 64, 2, True), (128, 256, 32, 32, 1, False)])
def test_h2_stride2_head_and_its_vjp_vs_float64(dev, f16x2, cin, cout, hs, ws, n, circular):
    """The level heads (3 x 3, stride 2: sda/nn.py:152-159) on conv_h2's per-class tap lists: forward over the four input parity planes
    (MODE 4), input VJP as four output parity classes of 1 / 2 / 2 / 4 taps with the skip gradient added (MODE 3) -- against float64
    (convolution / autograd) and against the fp32 kernels (direct implicit GEMM, conv_par4's zero-insertion form)."""
    from sda_amd import ops
    from sda_amd.engine import launch_conv, planar_source
    torch.manual_seed(cin + hs + 5 * ws)
    w = (torch.rand(cout, cin, 3, 3, device=dev) * 2 - 1) / math.sqrt(cin * 9)
    b = torch.randn(cout, device=dev)
    x = torch.randn(n, cin, hs, ws, device=dev) * 1.3
    # ---- forward
    pk = ops.PackedConv(w, b)
    assert pk.h2_s2() is not None
    x64 = x.double().cpu().requires_grad_(True)
    xp = F.pad(x64, (1, 1, 1, 1), mode='circular') if circular else F.pad(x64, (1, 1, 1, 1))
    ref = F.conv2d(xp, w.double().cpu(), b.double().cpu(), stride=2)
    out = torch.full((n, cout, hs // 2, ws // 2), float('nan'), device=dev)
    d = launch_conv(pk, planar_source(x), out, hs // 2, ws // 2, circular=circular, stride=(2, 2), bias=pk.bias, x_amax=ops.absmax(x, pk.in_amax))
    assert d.w_h2 and d.stride_h == 2, 'the stride-2 launch was not served by conv_h2'
    err = ((out.double().cpu() - ref.detach()).abs().max() / ref.abs().max()).item()
    out32 = torch.empty_like(out)
    d32 = launch_conv(pk, planar_source(x), out32, hs // 2, ws // 2, circular=circular, stride=(2, 2), bias=pk.bias)
    assert not d32.w_h2
    err32 = ((out32.double().cpu() - ref.detach()).abs().max() / ref.abs().max()).item()
    # ---- input VJP (+ the skip gradient)
    pkt = ops.PackedConv(w, None, transpose=True)
    assert pkt.h2_zins() is not None
    g = torch.randn(n, cout, hs // 2, ws // 2, device=dev) * 0.4
    skip = torch.randn(n, cin, hs, ws, device=dev)
    gref, = torch.autograd.grad(ref, x64, g.double().cpu())
    gref = gref + skip.double().cpu()
    gx = torch.full((n, cin, hs, ws), float('nan'), device=dev)
    dz = launch_conv(pkt, planar_source(g), gx, hs, ws, circular=circular, zins=(2, 2), res=skip, x_amax=ops.absmax(g, pkt.in_amax))
    assert dz.w_h2 and dz.zins_h == 2, 'the stride-2 VJP was not served by conv_h2'
    gerr = ((gx.double().cpu() - gref).abs().max() / gref.abs().max()).item()
    gx32 = torch.empty_like(gx)
    launch_conv(pkt, planar_source(g), gx32, hs, ws, circular=circular, zins=(2, 2), res=skip)
    gerr32 = ((gx32.double().cpu() - gref).abs().max() / gref.abs().max()).item()
    print(f'stride-2 head {cin}->{cout} @{hs}x{ws}: forward f16x2 {err:.2e} (fp32 kernel {err32:.2e}); VJP f16x2 {gerr:.2e} (fp32 kernel {gerr32:.2e})')
    assert err < 3e-6 and gerr < 3e-6


@pytest.mark.parametrize('cin,cout,hw,n', [(96, 96, 32, 2), (192, 192, 32, 2), (384, 384, 16, 2)])
def test_h2_trained_checkpoint_like_operands(dev, cin, cout, hw, n):
    """what a per-tensor power-of-two scale sees in a TRAINED net -- weights whose output channels carry scales spread
    log-uniformly over 1e-3 .. 1e1 (input channels 1e-1 .. 1e1: the small channels' `lo` halves land in f16's subnormal range) and
    activations with a 1 % heavy tail (cubed Gaussians, max |x| ~ 1e3 x typical).  Against float64: over the whole tensor (the suite's
    criterion, <= 3e-6 of max |ref|) AND per output channel relative to THAT channel's max |ref| (<= 4e-6: what the per-tensor scale
    could hide; the fp32 kernels on the same launches reach 0.6 - 2.3e-6, tools/h2_trained_like.py -> profiles/r06_h2_trained_like.txt)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('h2_trained_like', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                 'tools', 'h2_trained_like.py'))
    probe = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(probe)
    for kw in (dict(chan=False), dict(tail=False), {}):
        r = probe.run(cin, cout, hw, n, 11 + cin, **kw)
        served, whole, worst, _ = r['f16x2']
        assert served, 'the f16 x 2 kernel did not serve the launch'
        assert whole <= 3e-6 and worst <= 4e-6, (kw, r)
        assert worst <= 2.5 * r['f32'][2] + 1e-6, (kw, r)          # and in the fp32 kernels' class channel by channel


# the 16 rows of conv_h2's variant table (csrc/conv_h2.hip: H2_ROWS; tests/test_winograd_dispatch_host.py holds the table to the host pick)
H2_ROWS = [(ld, md, mb) for ld, md in ((0, 0), (1, 0), (2, 0), (0, 1), (2, 1), (0, 2), (0, 3), (0, 4)) for mb in (3, 2)]


@pytest.mark.parametrize('loader,mode,mb', H2_ROWS)
def test_h2_every_variant(dev, f16x2, loader, mode, mb):
    """Every instantiation of conv_h2_kernel runs once, at the smallest shape it admits (one 16 x 16 tile of 32 channels, 32 x 32 source
    pixels where the producers sample parity planes: the pooled and the stride-2 forms; 96 or 64 couts = the row's tile), against float64
    at the bound of this module's single launches."""
    from sda_amd import ops
    from sda_amd.engine import launch_conv, planar_source
    torch.manual_seed(10 * loader + 3 * mode + mb)
    k, m = 32, 32 * mb                                   # contraction channels, output channels of the LAUNCH
    transpose = mode in (2, 3)
    w = (torch.rand(k, m, 3, 3, device=dev) * 2 - 1) / math.sqrt(m * 9) if transpose else (torch.rand(m, k, 3, 3, device=dev) * 2 - 1) / math.sqrt(k * 9)
    b = None if transpose else torch.randn(m, device=dev)
    pk = ops.PackedConv(w, b, transpose=transpose)
    side = 32 if mode in (2, 4) else 16
    x = torch.randn(1, k, side, side, device=dev) * 1.3
    w64, x64 = w.double().cpu(), x.double().cpu()
    pad = lambda v: F.pad(v, (1, 1, 1, 1), mode='circular')
    kw, ln = {}, None
    if loader == 2:
        var, mean = torch.var_mean(x, dim=1, unbiased=True)
        ln = kw['ln'] = (mean.reshape(-1).contiguous(), (1 / torch.sqrt(var + 1e-5)).reshape(-1).contiguous())
    xa = None if ln is not None else ops.absmax(x, pk.in_amax)
    if mode == 0:
        res = torch.randn(1, m, side, side, device=dev)
        out = torch.full_like(res, float('nan'))
        d = launch_conv(pk, planar_source(x), out, side, side, circular=True, bias=pk.bias, act_in=1 if loader == 1 else 0, res=res, x_amax=xa, **kw)
        ref = _ref64(x, w, b, True, False, ln is not None, None, loader == 1, None, res)
        assert (d.up_h, d.pool_h, d.zins_h, d.stride_h) == (1, 1, 1, 1)
    elif mode == 1:
        out = torch.full((1, m, 2 * side, 2 * side), float('nan'), device=dev)
        d = launch_conv(pk, planar_source(x), out, 2 * side, 2 * side, circular=True, bias=pk.bias, up=(2, 2), x_amax=xa, **kw)
        if ln is not None:
            v64, m64 = torch.var_mean(x64, dim=1, unbiased=True, keepdim=True)
            x64 = (x64 - m64) / torch.sqrt(v64 + 1e-5)
        ref = F.conv2d(pad(x64.repeat_interleave(2, -1).repeat_interleave(2, -2)), w64, b.double().cpu())
        assert d.up_h == 2
    elif mode == 2:
        a64 = torch.zeros(1, m, side // 2, side // 2, dtype=torch.float64, requires_grad=True)
        ref, = torch.autograd.grad(F.conv2d(pad(a64.repeat_interleave(2, -1).repeat_interleave(2, -2)), w64), a64, x64)
        out = torch.full((1, m, side // 2, side // 2), float('nan'), device=dev)
        d = launch_conv(pk, planar_source(x), out, side, side, circular=True, pool=(2, 2), x_amax=xa)
        assert d is not None and d.pool_h == 2
    elif mode == 3:
        skip = torch.randn(1, m, 2 * side, 2 * side, device=dev)
        a64 = torch.zeros(1, m, 2 * side, 2 * side, dtype=torch.float64, requires_grad=True)
        ref, = torch.autograd.grad(F.conv2d(pad(a64), w64, stride=2), a64, x64)
        ref = ref + skip.double().cpu()
        out = torch.full_like(skip, float('nan'))
        d = launch_conv(pk, planar_source(x), out, 2 * side, 2 * side, circular=True, zins=(2, 2), res=skip, x_amax=xa)
        assert d.zins_h == 2
    else:
        out = torch.full((1, m, side // 2, side // 2), float('nan'), device=dev)
        d = launch_conv(pk, planar_source(x), out, side // 2, side // 2, circular=True, stride=(2, 2), bias=pk.bias, x_amax=xa)
        ref = F.conv2d(pad(x64), w64, b.double().cpu(), stride=2)
        assert d.stride_h == 2
    assert d.w_h2, 'the f16 x 2 kernel did not serve the launch'
    assert (d.cx, d.cout) == (k, m) and bool(d.ln_mean) == (loader == 2) and d.act_in == (1 if loader == 1 else 0)
    err = ((out.double().cpu() - ref).abs().max() / ref.abs().max()).item()
    assert err <= 3e-6, f'row {(loader, mode, mb)}: {err:.2e}'
