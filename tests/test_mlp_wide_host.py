"""CPU: the host side of the whole-MLP kernels at widths up to 256 (csrc/mlp1d.hip): slab sizes, the packing layout as include/sda_hip.h
words it, the planner's range."""
import numpy as np
import pytest
import torch

PIECE = 4096
UNSUPPORTED = -2


@pytest.fixture(scope='module')
def lib():
    from sda_amd import _lib
    return _lib.load()


def _narrow_floats(in_f, out_f):
    """The documented formula for both sides <= 128: [16 mf][16 kq] with mf = 1 / 8 (out <= 16 / 128), kq = 1 / 4 / 8 (in <= 16 / 64 / 128),
    zero padded to whole 4096-float pieces."""
    mf = 1 if out_f <= 16 else 8
    kq = 1 if in_f <= 16 else (4 if in_f <= 64 else 8)
    return -(-(mf * kq * 256) // PIECE) * PIECE


def test_slab_sizes(lib):
    for i in (1, 3, 15, 16, 17, 47, 63, 64, 65, 100, 127, 128):
        for o in (1, 15, 16, 17, 64, 100, 128):
            assert lib.sda_mlp_slab_floats(i, o) == _narrow_floats(i, o), (i, o)
    # the table of today's values, spelled out
    assert [lib.sda_mlp_slab_floats(i, o) for i, o in ((16, 16), (47, 128), (128, 128), (128, 15), (64, 16))] == [4096, 8192, 16384, 4096, 4096]
    for i in (1, 16, 47, 128, 129, 130, 192, 200, 255, 256):
        for o in (1, 15, 16, 17, 128, 129, 144, 200, 256):
            n = lib.sda_mlp_slab_floats(i, o)
            assert n > 0 and n % PIECE == 0, (i, o, n)
    assert lib.sda_mlp_slab_floats(256, 256) == 4 * 16384
    assert lib.sda_mlp_slab_floats(47, 256) == 2 * 8192 and lib.sda_mlp_slab_floats(256, 15) == 2 * 4096
    for i, o in ((257, 16), (16, 257), (257, 257), (0, 16), (16, 0)):
        assert lib.sda_mlp_slab_floats(i, o) == UNSUPPORTED, (i, o)


def _unit_matvec(unit, mf, kq, x):
    """y = Wp x from ONE unit, read as the header describes it: [m mf][sq kq][lane 64][4], element e of lane (k = lane >> 4, li = lane & 15)
    = Wp[16 m + li][16 sq + 4 k + e]."""
    y = np.zeros(16 * mf, dtype=np.float64)
    u = unit[:mf * kq * 256].reshape(mf, kq, 64, 4)
    for m in range(mf):
        for sq in range(kq):
            for lane in range(64):
                k, li = lane >> 4, lane & 15
                for e in range(4):
                    y[16 * m + li] += float(u[m, sq, lane, e]) * x[16 * sq + 4 * k + e]
    return y


def _slab_matvec(slab, in_f, out_f, x):
    """y = W x from a packed slab by the header's words: a side <= 128 pads to 16 / (64) / 128 and has one half, a side above 128 pads to
    256 and has two halves of 128; the units follow each other in the order [output half][input half], each padded to whole pieces."""
    pad_o = 16 if out_f <= 16 else (128 if out_f <= 128 else 256)
    pad_i = 16 if in_f <= 16 else (64 if in_f <= 64 else (128 if in_f <= 128 else 256))
    uo, ui = min(pad_o, 128), min(pad_i, 128)
    usz = -(-(uo * ui) // PIECE) * PIECE
    xp = np.zeros(pad_i)
    xp[:in_f] = x
    y = np.zeros(pad_o)
    u = 0
    for nh in range(pad_o // uo):
        for kh in range(pad_i // ui):
            y[uo * nh:uo * (nh + 1)] += _unit_matvec(slab[u * usz:(u + 1) * usz], uo // 16, ui // 16, xp[ui * kh:ui * (kh + 1)])
            u += 1
    assert u * usz == slab.size
    return y[:out_f], y[out_f:]


@pytest.mark.parametrize('out_f,in_f', [(256, 256), (200, 130), (15, 256), (256, 47), (144, 192), (129, 16), (100, 47)])
def test_packing_layout_matches_the_header(lib, out_f, in_f):
    from sda_amd import mlp
    rng = np.random.default_rng(out_f * 1000 + in_f)
    # small integers: every product and partial sum is exact in float32 and float64, so the comparison is exact
    W = rng.integers(-8, 9, size=(out_f, in_f)).astype(np.float32)
    x = rng.integers(-8, 9, size=in_f).astype(np.float64)
    for Wm, xv in ((W, x), (W.T.copy(), rng.integers(-8, 9, size=out_f).astype(np.float64))):      # the forward slab and the transposed one
        slab = mlp._slab(torch.from_numpy(Wm)).numpy()
        assert slab.size == lib.sda_mlp_slab_floats(Wm.shape[1], Wm.shape[0])
        y, tail = _slab_matvec(slab, Wm.shape[1], Wm.shape[0], xv)
        assert np.array_equal(y, Wm.astype(np.float64) @ xv)
        assert not tail.any()


def _plan(widths, acts=None, in_f=47, out_f=15):
    from sda_amd import mlp
    from sda_amd.nn import ResMLP
    from sda_amd.utils import ACTIVATIONS
    net = ResMLP(in_f, out_f, hidden_features=list(widths), activation=ACTIVATIONS['SiLU'])
    layers = list(net)
    if acts:
        blocks = [l for l in layers if not isinstance(l, torch.nn.Linear)]
        for blk, a in zip(blocks, acts):
            blk[2] = ACTIVATIONS[a]()
    return mlp._FusedPlan(layers)


def test_planner_range():
    p = _plan((256,) * 5)
    assert p.ok and len(p.gemms) == 14 and p.save_ld == 256      # (47 -> 256, five blocks, 256 -> 15, one block at 15)
    assert _plan((128,) * 5).ok and _plan((128,) * 5).save_ld == 128
    assert not _plan((257,)).ok
    assert not _plan((256, 257)).ok
    assert not _plan((256, 256), acts=('SiLU', 'ELU')).ok
    assert not _plan((256,) * 8).ok             # (20 GEMMs, 17 of them 256 wide: more padded bias than the kernel's 4096-float region holds)
    assert _plan((256,) * 7).ok
    p._pack()
    assert all(o % 4 == 0 for o in p.w_off + p.b_off)
    assert all(b > a for a, b in zip(p.w_off, p.w_off[1:])) and all(b > a for a, b in zip(p.b_off, p.b_off[1:]))
    lib = __import__('sda_amd._lib', fromlist=['load']).load()
    for g, (_k, i, o, _lin) in enumerate(p.gemms):
        end = p.w_off[g + 1] if g + 1 < len(p.gemms) else p.wf.numel()
        assert end - p.w_off[g] == max(lib.sda_mlp_slab_floats(i, o), lib.sda_mlp_slab_floats(o, i))
    assert p.bias.numel() == 11 * 256 + 3 * 16 and p.wf.numel() == p.wb.numel()
