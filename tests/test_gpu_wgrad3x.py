"""Device: the tiled weight-gradient kernel of the stride-2 heads and up-sampling tails (csrc/conv_wgrad3.hip, sda_conv_wgrad3x) through its C entry,
through ``ops.conv_wgrad(route='tiled_ht')`` and through a U-Net's backward under ``training.parameter_gradients(wgrad='tiled_ht')``.

Layer cases (tests/wgrad3x_cases.py), the widest served layers and a sample of tests/fuzz/wgrad3x_fuzz.py against the float64
reference of tests/wgrad_ref.py within 1e-5 of the largest element (test_gpu_wgrad3's layer bound); the net-level comparisons use
that file's net-level tolerances (1e-4 of the largest element of each gradient, the float64 oracle through
test_gpu_training._check_net, 1e-6 between chunked and unchunked)."""
import ctypes

import pytest
import torch
import torch.nn as nn

from oracle import sda_oracle as O
from sda_amd import engine as E
from sda_amd import ops, training
from sda_amd._lib import load as load_lib
from tests.util import rel_err
from tests.wgrad3x_cases import BOUNDARY, CASES, boundary_case, build
from tests.wgrad_ref import make_case, reference, wgrad_desc

pytestmark = pytest.mark.gpu

TOL = 1e-5


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def cases(dev):
    """name -> (case, float64 dW, float64 db): built once, never written."""
    out = {}
    for name in CASES:
        case = build(name, dev)
        out[name] = (case, *reference(case))
    return out


def launch(case, dev, route, slabs=0, accumulate=False, dw=None, db=None):
    cout, cin, kh, kw = case['cout'], case['v64'].shape[1], case['kh'], case['kw']
    dw = torch.full((cout, cin, kh, kw), float('nan'), device=dev) if dw is None else dw
    db = torch.full((cout,), float('nan'), device=dev) if db is None else db
    ops.conv_wgrad(case['conv'], case['g'], dw, db, accumulate, slabs, route=route)
    torch.cuda.synchronize()
    return dw, db


def device_wgrad3x(case, dev, slabs=0):
    """One launch of the C entry: dw / db start NaN-filled; ``work`` is NaN-filled to exactly the planned size, so an unwritten cell
    shows."""
    lib = load_lib()
    cout, cin = case['cout'], case['v64'].shape[1]
    dw = torch.full((cout, cin, 3, 3), float('nan'), device=dev)
    db = torch.full((cout,), float('nan'), device=dev)
    floats = int(lib.sda_conv_wgrad3x_work_floats(ctypes.byref(wgrad_desc(case, dw, db, slabs=slabs))))
    assert floats > 0, floats
    work = torch.full((floats,), float('nan'), device=dev)
    d = wgrad_desc(case, dw, db, work, slabs=slabs)
    assert lib.sda_conv_wgrad3x(ctypes.byref(d), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    return dw, db


def family_of(case, dev, route):
    prof = ops.ConvProfile()
    ops.conv_profile = prof
    try:
        launch(case, dev, route)
    finally:
        ops.conv_profile = None
    return [f for _a, _b, _fl, f in prof.records]


@pytest.mark.parametrize('name', list(CASES))
def test_layer_matches_float64_and_the_general_route(dev, cases, name):
    case, rw, rb = cases[name]
    assert family_of(case, dev, 'tiled_ht') == ['wgrad3x']
    assert family_of(case, dev, 'tiled') == ['wgrad'] and family_of(case, dev, 'general') == ['wgrad']
    dw, db = device_wgrad3x(case, dev)
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()
    print(name, 'tiled_ht vs float64: dw', rel_err(dw, rw), 'db', rel_err(db, rb))
    assert rel_err(dw, rw) <= TOL and rel_err(db, rb) <= TOL, (rel_err(dw, rw), rel_err(db, rb))
    dw2, db2 = device_wgrad3x(case, dev)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    ow, ob = launch(case, dev, 'tiled_ht')                                  # (the route the engine takes: same launch)
    assert torch.equal(dw, ow) and torch.equal(db, ob)
    gw, gb = launch(case, dev, 'general')
    print(name, 'tiled_ht vs general: dw', rel_err(dw, gw), 'db', rel_err(db, gb))
    assert rel_err(dw, gw) <= TOL and rel_err(db, gb) <= TOL, (rel_err(dw, gw), rel_err(db, gb))
    tw, tb = launch(case, dev, 'tiled')                                     # 'tiled' is still the general kernel here, bit for bit
    assert torch.equal(tw, gw) and torch.equal(tb, gb)


@pytest.mark.parametrize('name', ['up_ragged', 's2_workload_16'])
@pytest.mark.parametrize('slabs', [1, 3])
def test_layer_accumulates_onto_a_prior_with_forced_slabs(dev, cases, name, slabs):
    case, rw, rb = cases[name]
    dw, db = launch(case, dev, 'tiled_ht', slabs)
    assert rel_err(dw, rw) <= TOL and rel_err(db, rb) <= TOL, (rel_err(dw, rw), rel_err(db, rb))
    gen = torch.Generator().manual_seed(80 + slabs)
    pw, pb = (torch.randn(dw.shape, generator=gen) * 5).to(dev), (torch.randn(db.shape, generator=gen) * 5).to(dev)
    dw2, db2 = launch(case, dev, 'tiled_ht', slabs, accumulate=True, dw=pw.clone(), db=pb.clone())
    assert torch.equal(dw2, pw + dw) and torch.equal(db2, pb + db)
    dw3, db3 = launch(case, dev, 'tiled_ht', slabs, accumulate=True, dw=pw.clone(), db=pb.clone())
    assert torch.equal(dw2, dw3) and torch.equal(db2, db3)


@pytest.mark.parametrize('kind,cout', list(BOUNDARY))
def test_widest_served_layer_matches_float64(dev, kind, cout):
    """The kernel's largest LDS requests (just under 160 KiB): the widest layer of each geometry and cout tile, one row per stage."""
    case = boundary_case(kind, cout, dev)
    assert family_of(case, dev, 'tiled_ht') == ['wgrad3x']
    rw, rb = reference(case)
    dw, db = device_wgrad3x(case, dev)
    print(kind, cout, BOUNDARY[(kind, cout)], 'tiled_ht vs float64: dw', rel_err(dw, rw), 'db', rel_err(db, rb))
    assert rel_err(dw, rw) <= TOL and rel_err(db, rb) <= TOL, (rel_err(dw, rw), rel_err(db, rb))
    dw2, db2 = device_wgrad3x(case, dev)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize('kind,cout', list(BOUNDARY))
def test_one_past_the_widest_falls_back_to_the_general_kernel(dev, kind, cout):
    case = boundary_case(kind, cout, dev, over=1)
    assert family_of(case, dev, 'tiled_ht') == ['wgrad']
    dw, db = launch(case, dev, 'tiled_ht')
    gw, gb = launch(case, dev, 'general')
    assert torch.equal(dw, gw) and torch.equal(db, gb)
    rw, rb = reference(case)
    assert rel_err(dw, rw) <= TOL and rel_err(db, rb) <= TOL, (rel_err(dw, rw), rel_err(db, rb))


def test_block_convolution_keeps_its_kernel_under_tiled_ht(dev):
    case = make_case('conv1', dev, cin=32, cout=32, n=2, h=8, w=8, circular=True, seed=47)
    assert family_of(case, dev, 'tiled_ht') == ['wgrad3']
    dw, db = launch(case, dev, 'tiled_ht')
    tw, tb = launch(case, dev, 'tiled')
    assert torch.equal(dw, tw) and torch.equal(db, tb)


def test_wgrad3x_fuzz_sample(dev):
    """The draws of test_wgrad3x_host.test_wgrad3x_fuzz_sample on the device (tests/fuzz/wgrad3x_fuzz.py), each within 1e-5 of
    float64."""
    import random
    from tests.test_wgrad3x_host import FUZZ_CASES, FUZZ_SEED, load_wgrad3x_fuzz
    fuzz = load_wgrad3x_fuzz()
    device = fuzz.device()
    rng = random.Random(FUZZ_SEED)
    bad, worst = [], 0.0
    for i in range(FUZZ_CASES):
        spec = fuzz.draw_case(rng, i)
        dw, db, msg = fuzz.run_case(spec, device)
        if msg is None:
            ew, eb = fuzz.errors(spec, dw, db)
            worst = max(worst, ew, eb)
            if not (torch.isfinite(dw).all() and (db is None or torch.isfinite(db).all()) and ew <= fuzz.TOL and eb <= fuzz.TOL):
                msg = f'dw err {ew:.3e}, db err {eb:.3e}'
        if msg:
            bad.append((i, msg, spec['cfg']))
    print(f'wgrad3x fuzz sample: worst error vs float64 {worst:.3e}')
    assert not bad, '\n'.join(f'case {i}: {m}\n    {c}' for i, m, c in bad)


def test_the_c_entry_refuses_an_unserved_descriptor(dev):
    lib = load_lib()
    for case in (make_case('plain', dev, cin=32, cout=32, n=2, h=8, w=8, circular=False, seed=46),         # the other kernel's layer
                 make_case('head_s2', dev, cin=32, cout=32, n=2, h=7, w=8, circular=False, seed=46),       # odd source height
                 make_case('tail_up', dev, cin=32, cout=48, n=2, h=4, w=4, circular=True, seed=46)):
        cout = case['cout']
        dw, db = torch.full((cout, 32, 3, 3), float('nan'), device=dev), torch.full((cout,), float('nan'), device=dev)
        work = torch.zeros(1 << 16, device=dev)
        d = wgrad_desc(case, dw, db, work)
        assert lib.sda_conv_wgrad3x_serves(ctypes.byref(d)) == 0
        assert lib.sda_conv_wgrad3x(ctypes.byref(d), torch.cuda.current_stream().cuda_stream) == -2
        torch.cuda.synchronize()
        assert torch.isnan(dw).all() and torch.isnan(db).all()               # nothing was launched


# ---------------------------------------------------------------------------------------- net level

def _net(dev):
    from sda_amd.score import ScoreUNet
    torch.manual_seed(7)
    return ScoreUNet(3, embedding=16, hidden_channels=(32, 64), hidden_blocks=(1, 1), activation=nn.SiLU, spatial=2).to(dev)


def _grads(net, x, dev, profile=False, **switch):
    from sda_amd.score import VPSDE
    sde = VPSDE(net, shape=tuple(x.shape[1:])).to(dev)
    net.zero_grad(set_to_none=True)
    torch.manual_seed(23)
    prof = ops.ConvProfile() if profile else None
    ops.conv_profile = prof
    try:
        with training.parameter_gradients(**switch):
            sde.loss(x).backward()
        torch.cuda.synchronize()
    finally:
        ops.conv_profile = None
    grads = {k: p.grad.clone() for k, p in net.named_parameters()}
    return grads, (prof.summary()['families'] if profile else None)


def test_net_gradients_on_the_tiled_ht_route(dev):
    net = _net(dev)
    torch.manual_seed(9)
    x = torch.randn(2, 3, 16, 16, device=dev)
    general, fam_g = _grads(net, x, dev, profile=True, wgrad='general')
    tiled, fam_t = _grads(net, x, dev, profile=True, wgrad='tiled')
    ht, fam_h = _grads(net, x, dev, profile=True, wgrad='tiled_ht')
    assert 'wgrad3x' not in fam_g and 'wgrad3x' not in fam_t
    assert fam_h['wgrad3']['launches'] == fam_t['wgrad3']['launches']
    assert fam_h['wgrad3x']['launches'] == 2, fam_h                         # one head (32 -> 64, stride 2), one tail (64 -> 32, up 2)
    assert fam_h['wgrad']['launches'] == 2, fam_h                           # the first head and the last tail
    assert general.keys() == tiled.keys() == ht.keys()
    for k, ref in general.items():
        err = (ht[k].double() - ref.double()).abs().max().item()
        assert err <= 1e-4 * ref.abs().max().item() + 1e-12, f'{k}: {err:.3e} vs scale {ref.abs().max().item():.3e}'
    # the block convolutions take the same kernel with the same cotangents as under 'tiled'
    blocks = [k for k in ht if '.residue.' in k and ht[k].dim() in (1, 4)]
    assert len(blocks) == 16, blocks                                        # 4 blocks x 2 convolutions x (weight, bias)
    for k in blocks:
        assert torch.equal(ht[k], tiled[k]), k
    ht2, _ = _grads(net, x, dev, wgrad='tiled_ht')
    for k in ht:
        assert torch.equal(ht[k], ht2[k]), k


def test_default_switch_is_the_general_route_bitwise(dev):
    net = _net(dev)
    torch.manual_seed(9)
    x = torch.randn(2, 3, 16, 16, device=dev)
    default, fam = _grads(net, x, dev, profile=True)
    general, _ = _grads(net, x, dev, wgrad='general')
    assert 'wgrad3' not in fam and 'wgrad3x' not in fam
    for k in default:
        assert torch.equal(default[k], general[k]), k


# ---------------------------------------------------------------------------------------- the workload's widths, float64 oracle

WIDE = (96, 192)


def _wide_net(dev):
    from sda_amd.score import ScoreUNet
    torch.manual_seed(12)
    return ScoreUNet(3, embedding=16, hidden_channels=WIDE, hidden_blocks=(1, 1), activation=nn.SiLU, spatial=2,
                     padding_mode='circular').to(dev)


def test_wide_net_gradients_on_the_tiled_ht_route_match_the_float64_oracle(dev, monkeypatch):
    """The head 96 -> 192 and the tail 192 -> 96 on the new kernel at net level: every parameter gradient and the loss against
    torch.autograd of the oracle's float64 ``score_unet``, at test_gpu_training's net-level bounds."""
    from tests.test_gpu_training import _check_net, _kernel_eps
    from tests.test_gpu_wgrad3 import WgradLaunches
    net = _wide_net(dev)
    cfg = O.UNetConfig(3, 3, 16, WIDE, (1, 1), 3, 2, 'SiLU', 2, 'circular')
    torch.manual_seed(13)
    x = torch.randn(3, 3, 16, 16, device=dev)
    seen = WgradLaunches(monkeypatch)
    _check_net(net, (3, 16, 16), _kernel_eps(cfg), x, None, dev, wgrad='tiled_ht')
    new = [c for c in seen.calls if c[0] == 'wgrad3x']
    assert sorted(cout for _f, cout, _a in new) == [96, 192], seen.calls     # the tail's cout 96, the head's cout 192
    assert sum(f == 'wgrad' for f, _c, _a in seen.calls) == 2, seen.calls    # (first head, last tail: the general kernel)
    assert any(f == 'wgrad3' for f, _c, _a in seen.calls), seen.calls


def test_wide_net_chunked_recompute_on_the_tiled_ht_route(dev, monkeypatch):
    """Batch 6 recomputed in chunks of 2: the later chunks add into the gradient buffers (``accumulate``) on the new kernel."""
    from tests.test_gpu_training import _hip_grads
    from tests.test_gpu_wgrad3 import WgradLaunches
    net = _wide_net(dev)
    torch.manual_seed(14)
    x = torch.randn(6, 3, 16, 16, device=dev)
    _, g1, _, _ = _hip_grads(net, (3, 16, 16), x, None, 21, dev, wgrad='tiled_ht')
    g1 = {k: v.clone() for k, v in g1.items()}
    monkeypatch.setattr(E, 'KEEP_HBM_FRACTION', 1e-12)
    monkeypatch.setattr(E, 'CHUNK_HBM_FRACTION', 2.5 * net.network.engine().bytes_per_image(16, 16, True) /
                        torch.cuda.get_device_properties(dev).total_memory)
    seen = WgradLaunches(monkeypatch)
    _, g3, _, _ = _hip_grads(net, (3, 16, 16), x, None, 21, dev, wgrad='tiled_ht')
    new = [c for c in seen.calls if c[0] == 'wgrad3x']
    assert len(new) == 6 and sum(a for _f, _c, a in new) == 4, seen.calls    # head and tail, three chunks each: write, add, add
    assert any(cout == 192 and a for _f, cout, a in new) and any(cout == 96 and a for _f, cout, a in new), seen.calls
    for k in g1:
        assert rel_err(g3[k], g1[k]) <= 1e-6, (k, rel_err(g3[k], g1[k]))
