"""Device: the tiled 3 x 3 weight-gradient kernel (csrc/conv_wgrad3.hip) through ``ops.conv_wgrad(route='tiled')`` and through a
U-Net's backward under ``training.parameter_gradients(wgrad='tiled')``.

Layer cases (tests/wgrad3_cases.py) against the float64 reference of tests/wgrad_ref.py within the bound test_gpu_training.py uses
for the general kernel's layer cases (1e-5 of the largest element); the net-level comparison uses that file's net-level tolerance
(1e-4 of the largest element of each gradient)."""
import pytest
import torch
import torch.nn as nn

from sda_amd import ops, training
from tests.util import rel_err
from tests.wgrad3_cases import CASES, build
from tests.wgrad_ref import make_case, reference

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
    assert family_of(case, dev, 'tiled') == ['wgrad3'] and family_of(case, dev, 'general') == ['wgrad']
    dw, db = launch(case, dev, 'tiled')
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()
    print(name, 'tiled vs float64: dw', rel_err(dw, rw), 'db', rel_err(db, rb))
    assert rel_err(dw, rw) <= TOL and rel_err(db, rb) <= TOL, (rel_err(dw, rw), rel_err(db, rb))
    dw2, db2 = launch(case, dev, 'tiled')
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    gw, gb = launch(case, dev, 'general')
    print(name, 'tiled vs general: dw', rel_err(dw, gw), 'db', rel_err(db, gb))
    assert rel_err(dw, gw) <= TOL and rel_err(db, gb) <= TOL, (rel_err(dw, gw), rel_err(db, gb))


@pytest.mark.parametrize('slabs', [1, 3])
def test_layer_accumulates_onto_a_prior_with_forced_slabs(dev, cases, slabs):
    case, rw, rb = cases['wrap']
    dw, db = launch(case, dev, 'tiled', slabs)
    assert rel_err(dw, rw) <= TOL and rel_err(db, rb) <= TOL, (rel_err(dw, rw), rel_err(db, rb))
    gen = torch.Generator().manual_seed(80 + slabs)
    pw, pb = (torch.randn(dw.shape, generator=gen) * 5).to(dev), (torch.randn(db.shape, generator=gen) * 5).to(dev)
    dw2, db2 = launch(case, dev, 'tiled', slabs, accumulate=True, dw=pw.clone(), db=pb.clone())
    assert torch.equal(dw2, pw + dw) and torch.equal(db2, pb + db)
    dw3, db3 = launch(case, dev, 'tiled', slabs, accumulate=True, dw=pw.clone(), db=pb.clone())
    assert torch.equal(dw2, dw3) and torch.equal(db2, db3)
    # against float64: the prior in double plus the reference, at the scale of the sum
    assert rel_err(dw2, pw.double().cpu() + rw) <= TOL and rel_err(db2, pb.double().cpu() + rb) <= TOL


def test_ragged_row_block_and_ragged_last_slab(dev):
    # 14 rows in blocks of 12: the second block of every image has 2 live rows; 10 stages in 3 slabs of 4, 4, 2
    for circ in (True, False):
        case = make_case('conv1', dev, cin=32, cout=32, n=5, h=14, w=8, circular=circ, seed=44)
        rw, rb = reference(case)
        dw, db = launch(case, dev, 'tiled', 3)
        assert rel_err(dw, rw) <= TOL and rel_err(db, rb) <= TOL, (circ, rel_err(dw, rw), rel_err(db, rb))


def test_unserved_descriptor_falls_back_to_the_general_kernel(dev):
    case = make_case('head_s2', dev, cin=32, cout=32, n=2, h=8, w=8, circular=False, seed=46)
    assert family_of(case, dev, 'tiled') == ['wgrad']
    dw, db = launch(case, dev, 'tiled')
    gw, gb = launch(case, dev, 'general')
    assert torch.equal(dw, gw) and torch.equal(db, gb)
    rw, rb = reference(case)
    assert rel_err(dw, rw) <= TOL and rel_err(db, rb) <= TOL


def test_the_c_entry_refuses_an_unserved_descriptor(dev):
    import ctypes
    from sda_amd._lib import load
    from tests.wgrad_ref import wgrad_desc
    lib = load()
    case = make_case('head_s2', dev, cin=32, cout=32, n=2, h=8, w=8, circular=False, seed=46)
    dw, db = torch.full((32, 32, 3, 3), float('nan'), device=dev), torch.full((32,), float('nan'), device=dev)
    work = torch.zeros(1 << 16, device=dev)
    d = wgrad_desc(case, dw, db, work)
    assert lib.sda_conv_wgrad3_serves(ctypes.byref(d)) == 0
    assert lib.sda_conv_wgrad3(ctypes.byref(d), torch.cuda.current_stream().cuda_stream) == -2
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


def test_net_gradients_on_the_tiled_route(dev):
    net = _net(dev)
    torch.manual_seed(9)
    x = torch.randn(2, 3, 16, 16, device=dev)
    general, fam_g = _grads(net, x, dev, profile=True, wgrad='general')
    tiled, fam_t = _grads(net, x, dev, profile=True, wgrad='tiled')
    assert 'wgrad3' not in fam_g and fam_g['wgrad']['launches'] >= 1
    # the block convolutions (2 per block, 3 blocks) take the new route, the heads and tails the old one
    assert fam_t['wgrad3']['launches'] >= 1 and fam_t['wgrad']['launches'] >= 1, fam_t
    assert fam_t['wgrad3']['launches'] + fam_t['wgrad']['launches'] == fam_g['wgrad']['launches']
    assert general.keys() == tiled.keys()
    for k, ref in general.items():
        err = (tiled[k].double() - ref.double()).abs().max().item()
        assert err <= 1e-4 * ref.abs().max().item() + 1e-12, f'{k}: {err:.3e} vs scale {ref.abs().max().item():.3e}'
    tiled2, _ = _grads(net, x, dev, wgrad='tiled')
    for k in tiled:
        assert torch.equal(tiled[k], tiled2[k]), k


def test_default_switch_is_the_general_route_bitwise(dev):
    net = _net(dev)
    torch.manual_seed(9)
    x = torch.randn(2, 3, 16, 16, device=dev)
    default, fam = _grads(net, x, dev, profile=True)
    general, _ = _grads(net, x, dev, wgrad='general')
    assert 'wgrad3' not in fam
    for k in default:
        assert torch.equal(default[k], general[k]), k
