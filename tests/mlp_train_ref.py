"""Cases, descriptors and float64 references for the ResMLP weight-gradient entry points (csrc/mlp_train.hip), shared by the host
replay (tests/test_mlp_train_host.py) and the device tests (tests/test_gpu_mlp_train.py)."""
import ctypes

import torch

from sda_amd._lib import ACT_IDS, MlpWgradDesc

GUARD = 64                     # floats of NaN behind dw and behind db: the kernels must leave them NaN

ROWS = (1, 15, 16, 17, 63, 64, 65, 257)
SHAPES = ((47, 256), (256, 15), (15, 16), (17, 129), (128, 128), (256, 256))
KINDS = (0, 1, 2)

_ACT64 = {'SiLU': torch.nn.functional.silu, 'ReLU': torch.relu, 'ELU': torch.nn.functional.elu, 'GELU': torch.nn.functional.gelu,
          'SELU': torch.nn.functional.selu}


def make_case(rows, in_f, out_f, kind, dev='cpu', act='SiLU', seed=0):
    """One GEMM of a chain: G [rows][g_ld], the saved stream ``src`` [rows][src_ld] (row strides padded past the widths), and for kind 1
    the LayerNorm statistics; ``dw64`` / ``db64`` = float64 autograd of sum(G * (U W^T + b))."""
    gen = torch.Generator().manual_seed(1000 * seed + 7 * rows + 13 * in_f + 17 * out_f + kind)
    src_ld, g_ld = in_f + 3, out_f + 5
    src = torch.randn(rows, src_ld, generator=gen)
    g = torch.randn(rows, g_ld, generator=gen)
    mean = torch.randn(rows, generator=gen) * 0.3
    rstd = torch.rand(rows, generator=gen) + 0.5
    s64, g64 = src[:, :in_f].double(), g[:, :out_f].double()
    u = s64 if kind == 0 else ((s64 - mean.double()[:, None]) * rstd.double()[:, None] if kind == 1 else _ACT64[act](s64))
    w = torch.zeros(out_f, in_f, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(out_f, dtype=torch.float64, requires_grad=True)
    ((u @ w.t() + b) * g64).sum().backward()
    return dict(rows=rows, in_f=in_f, out_f=out_f, kind=kind, act=act, src=src.to(dev), g=g.to(dev), mean=mean.to(dev), rstd=rstd.to(dev),
                dw64=w.grad, db64=b.grad)


def buffers(cases, dev='cpu', fill=float('nan')):
    """dw / db of every case with GUARD floats behind each, all NaN."""
    return [(torch.full((c['out_f'] * c['in_f'] + GUARD,), fill, device=dev), torch.full((c['out_f'] + GUARD,), fill, device=dev)) for c in cases]


def wgrad_desc(cases, bufs, work=None, slabs=0, accumulate=False):
    """The sda_mlp_wgrad_desc of a chain whose GEMMs are ``cases`` (same rows, same g_ld is not required of the cases: the common g_ld is
    the first case's, so multi-GEMM chains use cases of one out_f)."""
    d = MlpWgradDesc()
    d.rows, d.ngemm, d.act = cases[0]['rows'], len(cases), ACT_IDS[cases[0]['act']]
    d.g_ld = cases[0]['g'].stride(0)
    for j, (c, (dw, db)) in enumerate(zip(cases, bufs)):
        assert c['g'].stride(0) == d.g_ld and c['rows'] == d.rows
        d.kind[j], d.in_f[j], d.out_f[j] = c['kind'], c['in_f'], c['out_f']
        d.src[j], d.src_ld[j] = c['src'].data_ptr(), c['src'].stride(0)
        d.mean[j], d.rstd[j] = c['mean'].data_ptr(), c['rstd'].data_ptr()
        d.g[j] = c['g'].data_ptr()
        d.dw[j], d.db[j] = dw.data_ptr(), db.data_ptr()
    d.work = None if work is None else work.data_ptr()
    d.slabs, d.accumulate = slabs, int(accumulate)
    return d


def bind(lib):
    for name, res in (('sda_mlp_wgrad_work_floats', ctypes.c_int64), ('sda_mlp_wgrad_slabs', ctypes.c_int)):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, [ctypes.POINTER(MlpWgradDesc)]
    return lib


def split(case, buf):
    """(dw [out][in], db [out], the two guard bands) of one case's buffers."""
    dw, db = buf
    n = case['out_f'] * case['in_f']
    return dw[:n].reshape(case['out_f'], case['in_f']), db[:case['out_f']], dw[n:], db[case['out_f']:]


def check_case(run, lib, case, dev='cpu', max_slabs=None):
    """The assertions every (rows, shape, kind) case gets, on the emulator or the device: ``run(desc)`` executes one descriptor.
    float64 agreement at 1e-5 of max |ref| under the planner's slab count; guard bands and nothing else stay NaN; ``work`` starts NaN;
    slabs 1, 2, 7 and the maximum are each bitwise repeatable and within the same bound; accumulate == prior + fresh, bitwise."""
    from tests.util import rel_err

    def once(slabs=0, accumulate=False, bufs=None):
        bufs = buffers([case], dev) if bufs is None else bufs
        floats = lib.sda_mlp_wgrad_work_floats(ctypes.byref(wgrad_desc([case], bufs, slabs=slabs)))
        assert floats > 0, floats
        work = torch.full((floats,), float('nan'), device=dev)
        run(wgrad_desc([case], bufs, work, slabs=slabs, accumulate=accumulate))
        return bufs[0]

    fresh = None
    for slabs in (0, 1, 2, 7, 64 if max_slabs is None else max_slabs):
        b1, b2 = once(slabs), once(slabs)
        dw, db, gw, gb = split(case, b1)
        assert torch.isnan(gw).all() and torch.isnan(gb).all(), 'guard band written'
        assert torch.isfinite(dw).all() and torch.isfinite(db).all()
        ew, eb = rel_err(dw, case['dw64']), rel_err(db, case['db64'])
        assert ew <= 1e-5 and eb <= 1e-5, (slabs, ew, eb)
        assert torch.equal(b1[0][:dw.numel()], b2[0][:dw.numel()]) and torch.equal(b1[1][:db.numel()], b2[1][:db.numel()]), slabs
        if slabs == 0:
            fresh = (dw.clone(), db.clone())
    prior = buffers([case], dev)
    pw, pb, _, _ = split(case, prior[0])
    gen = torch.Generator().manual_seed(3)
    pw.copy_(torch.randn(pw.shape, generator=gen))
    pb.copy_(torch.randn(pb.shape, generator=gen))
    want_w, want_b = pw.clone() + fresh[0], pb.clone() + fresh[1]
    once(0, True, prior)
    dw, db, gw, gb = split(case, prior[0])
    assert torch.equal(dw, want_w) and torch.equal(db, want_b)
    assert torch.isnan(gw).all() and torch.isnan(gb).all()
