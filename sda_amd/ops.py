"""Thin torch-tensor wrappers over the C ABI (include/sda_hip.h).

Every function launches a hand-written gfx950 kernel on the CURRENT torch stream.  There is no CPU path:
tensors must live on a HIP device (`_dev()` raises otherwise).
"""
import collections
import contextlib
import ctypes
import gc
import math
import os
from typing import Optional

import torch
from torch import Tensor

from . import _lib
from ._lib import ACT_IDS, ConvDesc

CONV_CK = 8          # K-stage depth of conv_igemm (SDA_CONV_CK)
WINOGRAD = os.environ.get('SDA_CONV_WINO', '1') != '0'      # 0: no Winograd form at all for the 3x3 layers
WINOGRAD4 = os.environ.get('SDA_CONV_WINO4', '1') != '0'    # 0: no conv_wino4 kernel (the one Winograd kernel: either switch means "direct kernel")
#: OPT-IN: 'f16x2' = the block convolutions multiply on the f16 matrix cores with every fp32 operand split into two halves, fp32
#: accumulation (csrc/conv_h2.hip; same 3e-7 error against float64 as the fp32 Winograd kernel).  Default 'f32': fp32 MFMAs only.
MULTIPLY = os.environ.get('SDA_MULTIPLY', 'f32')
if MULTIPLY not in ('f32', 'f16x2'):
    raise ValueError(f"SDA_MULTIPLY={MULTIPLY!r} (expected 'f32' or 'f16x2')")


def set_multiply(mode: str) -> str:
    """Select how the block convolutions multiply: 'f32' (default: fp32 MFMAs) or 'f16x2' (opt-in, csrc/conv_h2.hip).  Returns the
    previous mode.  Takes effect at the next evaluation (packed weights are keyed on it); not inside a captured graph."""
    global MULTIPLY
    if mode not in ('f32', 'f16x2'):
        raise ValueError(f"multiply mode {mode!r} (expected 'f32' or 'f16x2')")
    prev, MULTIPLY = MULTIPLY, mode
    return prev


#: f16 x 2 route: the up-sampled tails on conv_h2's parity-class form (SDA_H2_UP=0: the zero-position Winograd kernel, A/B runs)
H2_UP = os.environ.get('SDA_H2_UP', '1') != '0'
#: ... and their pooled VJP on the parity-plane form (SDA_H2_POOL=0: the zero-position Winograd kernel)
H2_POOL = os.environ.get('SDA_H2_POOL', '1') != '0'
#: ... and the stride-2 heads with their VJP on the per-class tap lists (SDA_H2_S2=0: the fp32 direct / conv_par4 kernels)
H2_S2 = os.environ.get('SDA_H2_S2', '1') != '0'


def tensor_version(t) -> int:
    """``t._version`` for cache keys; inference-mode tensors have no version counter (reading it raises) and cannot be written
    in place either, so a constant stands in for them."""
    return 0 if t is None or t.is_inference() else t._version


def _dev(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.SdaHipError('sda_amd ops run on MI355X only: got a CPU tensor (there is no CPU fallback)')
        if t.dtype != torch.float32:
            raise _lib.SdaHipError(f'sda_amd ops are fp32: got {t.dtype}')


def _ptr(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@contextlib.contextmanager
def capture_without_gc():
    """Around a stream capture: collect cyclic garbage first, and keep the collector off until the capture has ended.

    A generational collection that happens to start inside ``torch.cuda.graph`` runs the destructors of whatever dead device objects it
    finds -- an earlier sampler's graph with its private pool, streams, tensors held by a reference cycle -- and a runtime call made
    from there is illegal while a stream is capturing: the process aborts in the middle of the collection.  ``torch.cuda.graph`` itself
    no longer collects on entry, so when this happens depends on how many objects the process has allocated before."""
    was_enabled = gc.isenabled()
    gc.collect()
    gc.disable()
    try:
        yield
    finally:
        if was_enabled:
            gc.enable()


def round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def pick_mt(cout: int) -> int:
    """cout tile = 32*mt; choose the mt in 1..4 that wastes the fewest padded output channels."""
    best, best_pad = 1, None
    for mt in (3, 4, 2, 1):      # ties prefer 96-wide tiles: two double-buffered workgroups fit one CU's LDS
        pad = round_up(cout, 32 * mt)
        if best_pad is None or pad < best_pad:
            best, best_pad = mt, pad
    return best


def conv_out_size(size_v: int, k: int, stride: int) -> int:
    return (size_v + 2 * (k // 2) - k) // stride + 1


def make_conv_desc(*, x_ptr, n, cx, hs, ws, x_sc, x_sy, x_sx, x_sn_outer, x_sn_inner=0, n_inner=1, x_n_off=0,
                   w_ptr, cin_pad, cout_pad, cout, kh, kw, out_ptr, ho, wo, mt,
                   stride_h=1, stride_w=1, circular=False, up_h=1, up_w=1, zins_h=1, zins_w=1,
                   ctx_ptr=None, cctx=0, ctx_sn=0, mod_ptr=None, mod_sn=0, ln_mean_ptr=None, ln_rstd_ptr=None,
                   act_in=0, bias_ptr=None, dact_z_ptr=None, act_d=0, res_ptr=None,
                   w_wino4_ptr=None, pad=None, out_strides=(0, 0, 0, 0), pool=(1, 1), w_wino4_zp_ptr=None) -> ConvDesc:
    d = ConvDesc()
    d.x = x_ptr
    d.x_sn_outer, d.x_sn_inner, d.n_inner, d.x_n_off = x_sn_outer, x_sn_inner, n_inner, x_n_off
    d.x_sc, d.x_sy, d.x_sx = x_sc, x_sy, x_sx
    d.cx = cx
    d.ctx, d.ctx_sn, d.cctx = ctx_ptr, ctx_sn, cctx
    d.n, d.hs, d.ws = n, hs, ws
    d.up_h, d.up_w, d.zins_h, d.zins_w = up_h, up_w, zins_h, zins_w
    d.mod, d.mod_sn = mod_ptr, mod_sn
    d.ln_mean, d.ln_rstd = ln_mean_ptr, ln_rstd_ptr
    d.act_in = act_in
    d.kh, d.kw, d.stride_h, d.stride_w, d.circular = kh, kw, stride_h, stride_w, int(bool(circular))
    d.w, d.cin_pad, d.cout_pad = w_ptr, cin_pad, cout_pad
    d.bias = bias_ptr
    d.out, d.cout, d.ho, d.wo = out_ptr, cout, ho, wo
    d.dact_z, d.act_d = dact_z_ptr, act_d
    d.res = res_ptr
    d.mt = mt
    d.w_wino4 = w_wino4_ptr
    d.explicit_pad = 0 if pad is None else 1
    d.pad_h, d.pad_w = (0, 0) if pad is None else pad
    d.out_sn, d.out_sc, d.out_sy, d.out_sx = out_strides
    d.pool_h, d.pool_w = pool
    d.w_wino4_zp = w_wino4_zp_ptr
    return d


class ConvProfile:
    """Live timing of the kernels for bench.py's roofline leg: when installed as ``ops.conv_profile`` every conv_igemm
    launch is bracketed by HIP events on the launch stream and its ALGORITHMIC flops are recorded (2 * n * out-pixels *
    cout * cin * taps over the real channels; zero-inserted taps are not counted), by kernel family; the HBM-bound LayerNorm
    kernels are bracketed the same way with their algorithmic bytes (one read / write per operand)."""

    def __init__(self):
        self.records = []          # (start_event, stop_event, flops, family)
        self.family_bytes = {}     # family -> [algorithmic bytes read, written] over all its launches
        self.mem_records = []      # (start_event, stop_event, bytes, kernel)

    def flops(self, d: ConvDesc) -> float:
        pixels = d.ho * d.wo / (d.zins_h * d.zins_w)
        return 2.0 * d.n * pixels * d.cout * (d.cx + d.cctx) * d.kh * d.kw

    def alg_bytes(self, d: ConvDesc):
        """ALGORITHMIC bytes of a convolution launch: every operand read once (source, weights, LayerNorm statistics, epilogue
        operands), the output written once -- what the PMC traffic of profiles/*_traffic.json is compared against."""
        cin = d.cx + d.cctx
        rd = 4.0 * d.n * d.cx * d.hs * d.ws + 4.0 * d.cctx * d.hs * d.ws * (d.n if d.ctx_sn else 1)
        rd += 4.0 * cin * d.cout * (16 if d.w_wino4 and conv_path(d) in (2, 5) else d.kh * d.kw)
        if d.ln_mean:
            rd += 8.0 * d.n * d.hs * d.ws
        out = 4.0 * d.n * d.cout * d.ho * d.wo / (max(1, d.pool_h) * max(1, d.pool_w))
        rd += out * ((1 if d.res else 0) + (1 if d.dact_z else 0))
        return rd, out

    def conv_record(self, d: ConvDesc, family: str):
        """(family, flops, (bytes read, written)) of a served convolution launch."""
        # (a zero-insertion launch multiplies a quarter of what its fine-resolution output size says: 9 taps per SOURCE pixel)
        return family, self.flops(d) / float(max(1, d.zins_h) * max(1, d.zins_w)), self.alg_bytes(d)

    def bracket(self, family, flops: Optional[float], launch, nbytes=None):
        """The one place a launch is timed: ``launch()`` between two HIP events on the launch stream, then its record.  A launch
        that returns False was not served and ran nothing: no record.  ``flops`` None: an HBM-bound kernel with ``nbytes``
        algorithmic bytes (mem_records); else a compute family, ``nbytes`` = (read, written) adding to family_bytes.  ``family`` may
        be a callable -> (family, flops, nbytes), read once the launch is issued (a convolution's family is a planning call)."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        served = launch()
        if served is False:
            return False
        e1.record()
        if callable(family):
            family, flops, nbytes = family()
        if flops is None:
            self.mem_records.append((e0, e1, nbytes, family))
            return served
        self.records.append((e0, e1, flops, family))
        if nbytes is not None:
            b = self.family_bytes.setdefault(family, [0.0, 0.0])
            b[0] += nbytes[0]
            b[1] += nbytes[1]
        return served

    def bracket_mem(self, kernel: str, nbytes: float, launch):
        self.bracket(kernel, None, launch, nbytes)

    def mem_summary(self):
        torch.cuda.synchronize()
        out = {}
        for a, b, nb, k in self.mem_records:
            r = out.setdefault(k, dict(launches=0, ms=0.0, bytes=0.0))
            r['launches'] += 1
            r['ms'] += a.elapsed_time(b)
            r['bytes'] += nb
        return out

    def summary(self):
        torch.cuda.synchronize()
        out = dict(launches=len(self.records), total_ms=0.0, total_flops=0.0, families={})
        for a, b, f, fam in self.records:
            ms = a.elapsed_time(b)
            out['total_ms'] += ms
            out['total_flops'] += f
            r = out['families'].setdefault(fam, dict(launches=0, ms=0.0, flops=0.0))
            r['launches'] += 1
            r['ms'] += ms
            r['flops'] += f
        return out


conv_profile: Optional[ConvProfile] = None


def _bracketed(launch, record):
    """``launch()`` -- through the installed profile's bracket if there is one (bench.py's roofline leg); ``record()`` ->
    (family, flops, nbytes) as ConvProfile.bracket takes them is evaluated only then."""
    prof = conv_profile
    return launch() if prof is None else prof.bracket(record, None, launch)


def conv_igemm(desc: ConvDesc):
    lib = _lib.load()
    _bracketed(lambda: _lib.check(lib.sda_conv_igemm(ctypes.byref(desc), _stream()), 'sda_conv_igemm'),
               lambda: conv_profile.conv_record(desc, CONV_FAMILIES[max(0, conv_path(desc))]))


def absmax(x: Tensor, out: Tensor) -> Tensor:
    """out[0] = max |x| (device scalar; one streaming read of x): the input scale of an f16x2 launch whose producer did not report it."""
    _dev(x, out)
    if not x.is_contiguous():
        raise _lib.SdaHipError('absmax reads a contiguous tensor')
    _lib.check(_lib.load().sda_absmax(x.data_ptr(), x.numel(), out.data_ptr(), _stream()), 'sda_absmax')
    return out


def conv_h2(desc: ConvDesc, pk: 'PackedConv', x_amax, out_amax: Optional[Tensor], packing=None) -> bool:
    """Run the launch on the f16 x 2 kernel (csrc/conv_h2.hip) when `pk` carries that packing and the kernel serves the shape.
    x_amax: device scalar (Tensor) or a host bound (float) on the magnitude of what the loader feeds the multiply.  False: not
    served -- the caller runs the fp32 kernels."""
    if pk.h2 is None or x_amax is None:
        return False
    lib = _lib.load()
    if packing is None:
        desc.w_h2, desc.w_h2_scale = pk.h2.data_ptr(), pk.h2_scale
    else:                                                 # (buffer, scale): e.g. PackedConv.h2_up() for an up-sampled source
        desc.w_h2, desc.w_h2_scale = packing[0].data_ptr(), packing[1]
    if torch.is_tensor(x_amax):
        desc.x_amax, desc.x_amax_static = x_amax.data_ptr(), 0.0
    else:
        desc.x_amax, desc.x_amax_static = None, float(x_amax)
    desc.out_amax = None if out_amax is None else out_amax.data_ptr()
    if not lib.sda_conv_h2_supported(ctypes.byref(desc)):
        desc.w_h2 = None
        return False

    def launch():                                         # (the report slot is cleared inside the timed region)
        if out_amax is not None:
            out_amax.zero_()
        _lib.check(lib.sda_conv_h2(ctypes.byref(desc), _stream()), 'sda_conv_h2')
    # (the up-sampled / pooled forms issue 4 of the 9 taps; the stride-2 forms all 9, at a quarter of the fine-resolution pixels)
    _bracketed(launch, lambda: conv_profile.conv_record(
        desc, 'h2up' if (desc.up_h == 2 or desc.pool_h == 2) else 'h2s2' if (desc.zins_h == 2 or desc.stride_h == 2) else 'h2'))
    return True


PARITY4 = os.environ.get('SDA_CONV_PAR4', '1') != '0'
WINO4_BM64 = os.environ.get('SDA_W4_BM64', '1') != '0'      # 0: widths that are multiples of 32 but not of 96 stay on the direct kernel (A/B runs)


def conv_parity4(desc: ConvDesc) -> bool:
    """The four parity classes of a stride-2 3 x 3 convolution's backward-data in one launch (csrc/conv_par4.hip).  False: the
    shape is outside the kernel's range (the caller runs the four class launches)."""
    lib = _lib.load()

    def launch():
        rc = lib.sda_conv_parity4(ctypes.byref(desc), _stream())
        if rc == -2:                                     # SDA_E_UNSUPPORTED
            return False
        _lib.check(rc, 'sda_conv_parity4')
        return True

    def record():
        out = 16.0 * desc.n * desc.cout * desc.ho * desc.wo      # (desc: the class-(0, 0) quarter of the output)
        return ('par4', 2.0 * desc.n * desc.ho * desc.wo * desc.cout * desc.cx * 9,
                (4.0 * desc.n * desc.cx * desc.hs * desc.ws + 4.0 * 9 * desc.cx * desc.cout + (out if desc.res else 0.0), out))
    return _bracketed(launch, record)


POOLED = os.environ.get('SDA_CONV_POOLED', '1') != '0'


def conv_pooled(desc: ConvDesc) -> bool:
    """A convolution whose output is summed over pool_h x pool_w cells (sda_conv_desc.pool_h / pool_w).  False: no kernel serves
    the pooled form of this launch (the caller runs the plain launch and pools in its reader)."""
    lib = _lib.load()
    if lib.sda_conv_igemm_path(ctypes.byref(desc)) < 0:          # SDA_E_UNSUPPORTED: planning only, nothing launched
        return False
    conv_igemm(desc)
    return True


# indexed by sda_conv_igemm_path; slot 1 ('wino', the retired first-generation Winograd kernel) only keeps the indices: never returned
CONV_FAMILIES = ('direct', 'wino', 'wino4', 'small1d', 'few', 'wino4zp')


def conv_path(desc: ConvDesc) -> int:
    """Kernel family that would serve the launch: 2 Winograd (conv_wino4), 5 its zero-position form (2 x 2 up-sampled source or
    pooled output), 3 small 1-D kernel, 4 few-output-channel kernel, 0 direct implicit GEMM (1: retired, never returned)."""
    return _lib.load().sda_conv_igemm_path(ctypes.byref(desc))


def small1d_tile(desc: ConvDesc) -> int:
    """Positions per workgroup (16, 32 or 64) of the small 1-D kernel's launch serving ``desc``; 0 where the general kernels serve
    it (host only: nothing is launched, no pointer is followed)."""
    tile = _lib.load().sda_small1d_tile(ctypes.byref(desc))
    if tile < 0:
        _lib.check(tile, 'sda_small1d_tile')
    return tile


def pack_conv_weight(w: Tensor, cout: int, cin: int, kh: int, kw: int, transpose: bool, keep: int, dst: Tensor,
                     k_pad: int, m_pad: int):
    _lib.check(_lib.load().sda_pack_conv_weight(w.data_ptr(), cout, cin, kh, kw, int(transpose), keep, dst.data_ptr(),
                                                k_pad, m_pad, _stream()), 'sda_pack_conv_weight')



# ------------------------------------------------------------------------------------------ parameter gradients (csrc/conv_wgrad.hip)

def wgrad_desc(conv: ConvDesc, g: Tensor, dw: Tensor, db: Optional[Tensor], accumulate: bool, slabs: int = 0):
    """The sda_wgrad_desc of one layer: ``conv`` is the layer's FORWARD descriptor (how its loader read the input), ``g`` the
    cotangent at its output, planar contiguous [n][cout][ho][wo]; ``work`` is filled in by conv_wgrad."""
    d = _lib.WgradDesc()
    d.conv = conv
    d.g, d.dw, d.db = g.data_ptr(), dw.data_ptr(), _ptr(db)
    d.work = 1                                       # (placeholder for planning; conv_wgrad sets the real buffer)
    d.slabs, d.accumulate = slabs, int(bool(accumulate))
    return d


def wgrad_flops(conv: ConvDesc) -> float:
    return 2.0 * conv.n * conv.ho * conv.wo * conv.cout * (conv.cx + conv.cctx) * conv.kh * conv.kw


WGRAD_ROUTES = ('general', 'tiled', 'tiled_ht')


def conv_wgrad(conv: ConvDesc, g: Tensor, dw: Tensor, db: Optional[Tensor], accumulate: bool, slabs: int = 0, route: str = 'general'):
    """dw (+)= the weight gradient of the layer ``conv`` describes for the output cotangent ``g``; db (+)= its bias gradient.
    route 'tiled': the tiled 3 x 3 kernel (csrc/conv_wgrad3.hip) where sda_conv_wgrad3_serves says so, the general kernel otherwise;
    route 'tiled_ht': that, then the same kernel's heads' and tails' geometries where sda_conv_wgrad3x_serves says so, then the
    general kernel."""
    if route not in WGRAD_ROUTES:
        raise ValueError(f"conv_wgrad route {route!r} (expected 'general', 'tiled' or 'tiled_ht')")
    _dev(g, dw, db)
    if not g.is_contiguous() or tuple(g.shape) != (conv.n, conv.cout, conv.ho, conv.wo):
        raise _lib.SdaHipError(f'conv_wgrad: cotangent must be planar contiguous {(conv.n, conv.cout, conv.ho, conv.wo)}, got {tuple(g.shape)}')
    cin = conv.cx + conv.cctx
    if not dw.is_contiguous() or dw.numel() != conv.cout * cin * conv.kh * conv.kw or (db is not None and db.numel() != conv.cout):
        raise _lib.SdaHipError('conv_wgrad: dw / db do not match the layer')
    lib = _lib.load()
    d = wgrad_desc(conv, g, dw, db, accumulate, slabs)
    if route != 'general' and lib.sda_conv_wgrad3_serves(ctypes.byref(d)):
        planner, launch, name, family = lib.sda_conv_wgrad3_work_floats, lib.sda_conv_wgrad3, 'sda_conv_wgrad3', 'wgrad3'
    elif route == 'tiled_ht' and lib.sda_conv_wgrad3x_serves(ctypes.byref(d)):
        planner, launch, name, family = lib.sda_conv_wgrad3x_work_floats, lib.sda_conv_wgrad3x, 'sda_conv_wgrad3x', 'wgrad3x'
    else:
        planner, launch, name, family = lib.sda_conv_wgrad_work_floats, lib.sda_conv_wgrad, 'sda_conv_wgrad', 'wgrad'
    floats = planner(ctypes.byref(d))
    _lib.check(int(min(floats, 0)), name + '_work_floats')
    work = torch.empty(int(floats), device=g.device, dtype=torch.float32)
    d.work = work.data_ptr()
    _bracketed(lambda: _lib.check(launch(ctypes.byref(d), _stream()), name), lambda: (family, wgrad_flops(conv), None))


def plane_sum(x: Tensor, y: Optional[Tensor], out: Tensor, out_sn: int, sum_images: bool, accumulate: bool):
    """out[i * out_sn + ch] (+)= sum over the plane of (x - y)[i][ch] (x, y planar [n][c][...]); sum_images: out[ch] (+)= over all i."""
    _dev(x, y, out)
    if not x.is_contiguous() or (y is not None and (not y.is_contiguous() or y.shape != x.shape)):
        raise _lib.SdaHipError('plane_sum: operands must be planar contiguous and alike')
    n, c = x.shape[0], x.shape[1]
    hw = x[0, 0].numel()

    def launch():
        _lib.check(_lib.load().sda_plane_sum(x.data_ptr(), _ptr(y), n, c, hw, out.data_ptr(), out_sn, int(bool(sum_images)),
                                             int(bool(accumulate)), _stream()), 'sda_plane_sum')
    _bracketed(launch, lambda: ('plane_sum', None, 4.0 * n * c * hw * (2 if y is not None else 1)))

class PackedConv:
    """A conv layer's weights repacked for sda_conv_igemm (forward or backward-data form)."""

    def __init__(self, weight: Tensor, bias: Optional[Tensor], transpose: bool = False, cin_keep: Optional[int] = None):
        _dev(weight, bias)
        w = weight.detach().contiguous()
        cout, cin = w.shape[0], w.shape[1]
        ks = tuple(w.shape[2:])
        self.kh, self.kw = (1, ks[0]) if len(ks) == 1 else ks
        self._transpose = bool(transpose)
        self._w_ref = w if (MULTIPLY == 'f16x2' and len(ks) == 2) else None     # (h2_up() sums taps of the original layout on first use)
        self._h2_up = None
        self._h2_pool = None
        self._h2_zins = None
        self._h2_s2 = None
        if transpose:
            keep = cin if cin_keep is None else cin_keep
            self.k_real, self.m_real = cout, keep          # contraction over forward cout, produces forward cin
        else:
            keep = cin
            self.k_real, self.m_real = cin, cout
        self.mt = pick_mt(self.m_real)
        self.k_pad = round_up(self.k_real, CONV_CK)
        self.m_pad = round_up(self.m_real, 32 * self.mt)
        self.packed = torch.empty(self.kh * self.kw * self.k_pad * self.m_pad, device=w.device, dtype=torch.float32)
        pack_conv_weight(w, cout, cin, self.kh, self.kw, transpose, keep, self.packed, self.k_pad, self.m_pad)
        self.bias = None if (bias is None or transpose) else bias.detach().contiguous()
        # Winograd F(2x2,3x3) form for the 3x3 layers (conv_wino4.hip: U fragments in MFMA lane order).  Its cout tile is 96 where the
        # width allows (the reference's training widths (96, 192, 384)), 64 for the other multiples of 64 -- the reference's DEFAULT
        # widths (64, 128, 256), experiments/kolmogorov/utils.py:52 -- and 32 for the remaining multiples of 32 (UNet's own default
        # (32, 64, 128), sda/nn.py:99)
        self.wino4 = None
        if (WINOGRAD and WINOGRAD4 and (self.kh, self.kw) == (3, 3) and self.m_pad == self.m_real and
                (self.m_real % 96 == 0 or (WINO4_BM64 and self.m_real % 32 == 0))):
            self.wino4 = torch.empty(16 * self.k_pad * self.m_pad, device=w.device, dtype=torch.float32)
            _lib.check(_lib.load().sda_pack_conv_weight_wino4(w.data_ptr(), cout, cin, int(transpose), keep,
                                                              self.wino4.data_ptr(), self.k_pad, self.m_pad, _stream()),
                       'sda_pack_conv_weight_wino4')
        # ... and its zero-position packing (sda_pack_conv_weight_wino4_zp: the 9 live Winograd positions of a 2 x 2 up-sampled / pooled
        # launch, 28 KiB per K stage and cout tile instead of 36) -- made here, not on first use: a launch must not allocate (its operands
        # may be views of freed temporaries the allocator would hand out again; a step may be under graph capture)
        self._wino4_zp = None
        if self.wino4 is not None:
            lib = _lib.load()
            self._wino4_zp = torch.empty(int(lib.sda_wino4_zp_floats(self.k_pad, self.m_pad)), device=w.device, dtype=torch.float32)
            _lib.check(lib.sda_pack_conv_weight_wino4_zp(self.wino4.data_ptr(), self.k_pad, self.m_pad, self._wino4_zp.data_ptr(), _stream()),
                       'sda_pack_conv_weight_wino4_zp')

        # ... and, OPT-IN (ops.MULTIPLY == 'f16x2'), the two-halves packing of csrc/conv_h2.hip with its scale (max |w| is read back
        # once, here -- packing happens in warm-up, never under graph capture) and the device scalars its launches report through
        self.h2 = None
        if MULTIPLY == 'f16x2' and (self.kh, self.kw) == (3, 3) and (not transpose or keep == cin) and w.numel() > 0:
            lib = _lib.load()
            nbytes = int(lib.sda_conv_h2_packed_bytes(cout, cin, int(transpose)))
            if nbytes > 0:
                w_amax = float(w.abs().max())
                if w_amax > 0.0 and math.isfinite(w_amax):
                    self.h2 = torch.empty(nbytes, device=w.device, dtype=torch.uint8)
                    _lib.check(lib.sda_pack_conv_weight_h2(w.data_ptr(), cout, cin, int(transpose), w_amax, self.h2.data_ptr(), _stream()),
                               'sda_pack_conv_weight_h2')
                    self.h2_scale = float(lib.sda_conv_h2_scale(w_amax))
                    self.out_amax = torch.zeros(1, device=w.device, dtype=torch.float32)     # max |out| of this layer's last launch
                    self.in_amax = torch.zeros(1, device=w.device, dtype=torch.float32)      # scratch for an absmax pass over its input

    def _h2_wsum(self) -> Tensor:
        """[4 classes (2 py + px)][cout][cin][4 taps (2 a + b)]: the 3 x 3 taps that read ONE source pixel of a 2 x 2 nearest-up-sampled image,
        summed (fp32) -- output pixel (2 i + py, 2 j + px) sees source rows i - 1 + py + a: py = 0: dy {0} | {1, 2}; py = 1: {0, 1} | {2}."""
        w = self._w_ref                                        # [cout][cin][3][3], the layer's own layout
        cout, cin = w.shape[0], w.shape[1]
        rows = (((0,), (1, 2)), ((0, 1), (2,)))
        wsum = torch.empty(4, cout, cin, 4, device=w.device, dtype=torch.float32)
        for py in range(2):
            for px in range(2):
                for a_ in range(2):
                    for b_ in range(2):
                        acc = None
                        for dy in rows[py][a_]:
                            for dx in rows[px][b_]:
                                acc = w[:, :, dy, dx] if acc is None else acc + w[:, :, dy, dx]
                        wsum[2 * py + px, :, :, 2 * a_ + b_] = acc
        return wsum

    def h2_up(self):
        """(packing, scale) of the f16 x 2 form over a 2 x 2 nearest-up-sampled source (sda_pack_conv_weight_h2_up), or None: the four
        output parity classes as 2 x 2-tap convolutions with pre-summed taps.  Built on first use (warm-up, never under capture)."""
        if self.h2 is None or self._transpose or getattr(self, '_w_ref', None) is None:
            return None
        if getattr(self, '_h2_up', None) is None:
            lib = _lib.load()
            cout, cin = self._w_ref.shape[0], self._w_ref.shape[1]
            nbytes = int(lib.sda_conv_h2_up_packed_bytes(cout, cin))
            self._h2_up = False
            if nbytes > 0:
                wsum = self._h2_wsum()
                amax = float(wsum.abs().max())
                if amax > 0.0 and math.isfinite(amax):
                    buf = torch.empty(nbytes, device=wsum.device, dtype=torch.uint8)
                    _lib.check(lib.sda_pack_conv_weight_h2_up(wsum.data_ptr(), cout, cin, amax, buf.data_ptr(), _stream()),
                               'sda_pack_conv_weight_h2_up')
                    torch.cuda.current_stream(wsum.device).synchronize()      # (wsum is a temporary)
                    self._h2_up = (buf, float(lib.sda_conv_h2_scale(amax)))
        return self._h2_up or None

    def h2_pool(self):
        """(packing, scale) for the VJP of such a tail summed over the 2 x 2 up-sampling cells (this object is the layer's backward-data
        form): a 2 x 2-tap convolution over the four parity planes of the fine-resolution gradient (sda_pack_conv_weight_h2_rows), or None."""
        if self.h2 is None or not self._transpose or getattr(self, '_w_ref', None) is None:
            return None
        if getattr(self, '_h2_pool', None) is None:
            lib = _lib.load()
            cout, cin = self._w_ref.shape[0], self._w_ref.shape[1]
            nbytes = int(lib.sda_conv_h2_rows_packed_bytes(cin, 4 * cout, 4)) if self.m_real == cin else 0
            self._h2_pool = False
            if nbytes > 0:
                wrows = self._h2_wsum().permute(2, 0, 1, 3).reshape(cin, 4 * cout, 4).contiguous()      # [ci][class * cout + co][tap]
                amax = float(wrows.abs().max())
                if amax > 0.0 and math.isfinite(amax):
                    buf = torch.empty(nbytes, device=wrows.device, dtype=torch.uint8)
                    _lib.check(lib.sda_pack_conv_weight_h2_rows(wrows.data_ptr(), cin, 4 * cout, 4, amax, buf.data_ptr(), _stream()),
                               'sda_pack_conv_weight_h2_rows')
                    torch.cuda.current_stream(wrows.device).synchronize()
                    self._h2_pool = (buf, float(lib.sda_conv_h2_scale(amax)))
        return self._h2_pool or None

    def _h2_classes(self, vjp: bool):
        """(packing, scale) of a STRIDE-2 3 x 3 layer on conv_h2's per-class tap lists (csrc/conv_h2.hip MODE 3 / 4): class (py, px) has the
        taps dy in ((1,), (0, 2))[py], dx alike -- 1 / 2 / 2 / 4 of the layer's 9 -- packed class after class by
        sda_pack_conv_weight_h2_rows; vjp: rows = forward cin, K = forward cout (the input VJP), else the forward orientation."""
        lib = _lib.load()
        w = self._w_ref                                        # [cout][cin][3][3]
        cout, cin = w.shape[0], w.shape[1]
        rows, k = (cin, cout) if vjp else (cout, cin)
        sizes = [int(lib.sda_conv_h2_rows_packed_bytes(rows, k, (1 + (c >> 1)) * (1 + (c & 1)))) for c in range(4)]
        amax = float(w.abs().max())
        if min(sizes) <= 0 or not (amax > 0.0 and math.isfinite(amax)):
            return False
        buf = torch.empty(sum(sizes), device=w.device, dtype=torch.uint8)
        taps = ((1,), (0, 2))
        off = 0
        for c in range(4):
            wc = torch.stack([w[:, :, dy, dx] for dy in taps[c >> 1] for dx in taps[c & 1]], dim=-1)      # [cout][cin][nt]
            if vjp:
                wc = wc.permute(1, 0, 2)
            wc = wc.contiguous()
            _lib.check(lib.sda_pack_conv_weight_h2_rows(wc.data_ptr(), rows, k, wc.shape[-1], amax, buf[off:].data_ptr(), _stream()),
                       'sda_pack_conv_weight_h2_rows')
            torch.cuda.current_stream(w.device).synchronize()  # (wc is a temporary)
            off += sizes[c]
        return (buf, float(lib.sda_conv_h2_scale(amax)))

    def h2_zins(self):
        """The input VJP of a stride-2 3 x 3 layer (this object is its backward-data form) on conv_h2's parity-class form, or None."""
        if self.h2 is None or not self._transpose or getattr(self, '_w_ref', None) is None or self.m_real != self._w_ref.shape[1]:
            return None
        if getattr(self, '_h2_zins', None) is None:
            self._h2_zins = self._h2_classes(True)
        return self._h2_zins or None

    def h2_s2(self):
        """A stride-2 3 x 3 layer on conv_h2's parity-plane form (forward), or None."""
        if self.h2 is None or self._transpose or getattr(self, '_w_ref', None) is None:
            return None
        if getattr(self, '_h2_s2', None) is None:
            self._h2_s2 = self._h2_classes(False)
        return self._h2_s2 or None

    def wino4_zp(self) -> Optional[Tensor]:
        """The zero-position packing of `wino4` (None without it): what the up-sampling tails (sda/nn.py:161-169 of the reference) and
        their VJPs multiply with."""
        return self._wino4_zp


# ------------------------------------------------------------------------------------------ fused 1-D residual block

BLOCK1D = os.environ.get('SDA_BLOCK1D', '1') != '0'


def block1d_eligible(c: int, h: int, pk1: 'PackedConv', pk2: 'PackedConv') -> bool:
    """One-launch residual block (block1d.hip): 1-D, <= 64 channels, two k = 3 stride-1 convolutions c -> c."""
    return (BLOCK1D and h == 1 and 2 <= c <= 64 and (pk1.kh, pk1.kw) == (1, 3) and (pk2.kh, pk2.kw) == (1, 3) and
            pk1.k_pad <= 64 and pk1.m_pad <= 64 and pk2.k_pad == pk1.k_pad and pk2.m_pad == pk1.m_pad and
            pk1.k_real == c and pk1.m_real == c and pk2.k_real == c and pk2.m_real == c)


def _bracket_block1d(family: str, d, launch):
    """bench.py's roofline leg: a fused 1-D residual block is two k = 3 convolutions c -> c over n x len positions."""
    _bracketed(launch, lambda: (family, 2 * (2.0 * d.n * d.len * d.c * d.c * 3), None))


def _block1d_desc(a, mod, mod_sn, pk1, pk2, circular, act, eps, unbiased):
    d = _lib.Block1dDesc()
    d.n, d.c, d.len = a.shape[0], a.shape[1], a.shape[-1]
    d.circular, d.act, d.unbiased, d.eps = int(circular), act, int(unbiased), eps
    d.k_pad, d.m_pad = pk1.k_pad, pk1.m_pad
    d.a = a.data_ptr()
    d.mod, d.mod_sn = _ptr(mod), mod_sn
    d.w1, d.w2 = pk1.packed.data_ptr(), pk2.packed.data_ptr()
    d.b1 = None if pk1.bias is None else pk1.bias.data_ptr()
    d.b2 = None if pk2.bias is None else pk2.bias.data_ptr()
    return d


def block1d_fwd(a: Tensor, mod, mod_sn: int, pk1: 'PackedConv', pk2: 'PackedConv', circular: bool, act: int, eps: float,
                unbiased: bool, y: Tensor, z: Optional[Tensor] = None, mean: Optional[Tensor] = None,
                rstd: Optional[Tensor] = None):
    """y = a + conv2(act(conv1(LN(a + mod)))) for planar a (n, c, 1, len); z / mean / rstd are kept for the VJP when given."""
    _dev(a, mod, y, z, mean, rstd)
    d = _block1d_desc(a, mod, mod_sn, pk1, pk2, circular, act, eps, unbiased)
    d.y, d.z, d.mean, d.rstd = y.data_ptr(), _ptr(z), _ptr(mean), _ptr(rstd)
    _bracket_block1d('block1d_fwd', d, lambda: _lib.check(_lib.load().sda_block1d_fwd(ctypes.byref(d), _stream()), 'sda_block1d_fwd'))


def block1d_bwd(g: Tensor, a: Tensor, z: Tensor, mean: Tensor, rstd: Tensor, mod, mod_sn: int, pk1b: 'PackedConv',
                pk2b: 'PackedConv', circular: bool, act: int, unbiased: bool, gx: Tensor):
    """gx = g + LN^T(conv1^T(act'(z) . conv2^T(g))); pk1b / pk2b: the backward-data packings."""
    _dev(g, a, z, mean, rstd, mod, gx)
    d = _block1d_desc(a, mod, mod_sn, pk1b, pk2b, circular, act, 0.0, unbiased)
    d.z, d.mean, d.rstd, d.g, d.gx = z.data_ptr(), mean.data_ptr(), rstd.data_ptr(), g.data_ptr(), gx.data_ptr()
    _bracket_block1d('block1d_bwd', d, lambda: _lib.check(_lib.load().sda_block1d_bwd(ctypes.byref(d), _stream()), 'sda_block1d_bwd'))


def block1d_tile(d: '_lib.Block1dDesc') -> int:
    """Positions per workgroup (16, 32 or 64) of the block1d launch serving ``d``, forward and VJP alike (host only: the shape
    fields decide, pointers may be unset)."""
    tile = _lib.load().sda_block1d_tile(ctypes.byref(d))
    if tile < 1:
        _lib.check(tile, 'sda_block1d_tile')
    return tile


# ------------------------------------------------------------------------------------------ whole single-level 1-D net

NET1D = os.environ.get('SDA_NET1D', '1') != '0'


def net1d_launch(d: '_lib.Net1dDesc', backward: bool):
    """One launch for a whole single-level 1-D U-Net (csrc/net1d.hip), forward or input VJP; see include/sda_hip.h.
    (engine.net1d_plan mirrors the kernel's eligibility checks, so SDA_E_UNSUPPORTED here is a planning bug and raises.)"""
    lib = _lib.load()
    fn, name = (lib.sda_net1d_bwd, 'sda_net1d_bwd') if backward else (lib.sda_net1d_fwd, 'sda_net1d_fwd')
    _net1d_bracket('net1d_bwd' if backward else 'net1d_fwd', d, lambda: _lib.check(fn(ctypes.byref(d), _stream()), name))


def _net1d_bracket(tag: str, d: '_lib.Net1dDesc', launch):
    """The whole net's convolutions: head, two per block, tail, k = 3 each."""
    _bracketed(launch, lambda: (tag, 2.0 * d.n * d.len * 3 * (d.cin * d.c + 2 * d.nblocks * d.c * d.c + d.c * d.cout), None))


def net1d_fwd_train(t: '_lib.Net1dTrainDesc'):
    """sda_net1d_fwd with the saves of a training step (csrc/net1d_train.hip): also writes the tail convolution's input."""
    lib = _lib.load()
    _net1d_bracket('net1d_fwd', t.net, lambda: _lib.check(lib.sda_net1d_fwd_train(ctypes.byref(t), _stream()), 'sda_net1d_fwd_train'))


def net1d_bwd_train(t: '_lib.Net1dTrainDesc'):
    """sda_net1d_bwd that also stores every convolution's output cotangent and the per-tile modulation-gradient sums."""
    lib = _lib.load()
    _net1d_bracket('net1d_bwd', t.net, lambda: _lib.check(lib.sda_net1d_bwd_train(ctypes.byref(t), _stream()), 'sda_net1d_bwd_train'))


def net1d_tiles(d: '_lib.Net1dDesc') -> int:
    """Tiles per sequence of the whole-net launch serving ``d`` (host only)."""
    tiles = _lib.load().sda_net1d_tiles(ctypes.byref(d))
    if tiles < 1:
        _lib.check(tiles, 'sda_net1d_tiles')
    return tiles


def net1d_wgrad(d: '_lib.Net1dWgradDesc', device) -> Tensor:
    """Weight, bias and modulation gradients of a whole single-level 1-D U-Net: one multiply launch over all convolutions + one
    ordered slab reduction (sda_net1d_wgrad).  Allocates the slab partials (d.work) and returns them (the caller keeps them alive
    no longer than the stream order needs: torch's caching allocator is stream-ordered)."""
    lib = _lib.load()
    floats = int(lib.sda_net1d_wgrad_work_floats(ctypes.byref(d)))
    if floats < 0:
        _lib.check(floats, 'sda_net1d_wgrad_work_floats')
    work = torch.empty(floats, device=device, dtype=torch.float32)
    d.work = work.data_ptr()
    _net1d_bracket('net1d_wgrad', d.net, lambda: _lib.check(lib.sda_net1d_wgrad(ctypes.byref(d), _stream()), 'sda_net1d_wgrad'))
    return work


def net1d_pack(p: '_lib.Net1dPackDesc'):
    """Every packing of a whole-net launch (forward buffer, backward-data buffer, bias rows: the non-NULL ones) in one launch."""
    _lib.check(_lib.load().sda_net1d_pack(ctypes.byref(p), _stream()), 'sda_net1d_pack')


def net1d_launch_fused(d: '_lib.Net1dDesc', f: '_lib.Net1dFuse', backward: bool):
    """One half of a fused guided evaluation (sda_net1d_fwd_fused / sda_net1d_bwd_fused; sda_amd/fused1d.py)."""
    lib = _lib.load()
    fn, name = (lib.sda_net1d_bwd_fused, 'sda_net1d_bwd_fused') if backward else (lib.sda_net1d_fwd_fused, 'sda_net1d_fwd_fused')
    _net1d_bracket('net1d_bwd' if backward else 'net1d_fwd', d, lambda: _lib.check(fn(ctypes.byref(d), ctypes.byref(f), _stream()), name))


# ------------------------------------------------------------------------------------------ LayerNorm pieces

def ln_stats(x: Tensor, mod: Optional[Tensor], mod_sn: int, eps: float, unbiased: bool, mean: Tensor, rstd: Tensor):
    """x: planar [n][c][hw] contiguous."""
    _dev(x, mod, mean, rstd)
    n, c = x.shape[0], x.shape[1]
    hw = x[0, 0].numel()

    def launch():
        _lib.check(_lib.load().sda_ln_stats(x.data_ptr(), n, c, hw, _ptr(mod), mod_sn, eps, int(unbiased),
                                            mean.data_ptr(), rstd.data_ptr(), _stream()), 'sda_ln_stats')
    _bracketed(launch, lambda: ('ln_stats', None, 4.0 * n * hw * (c + 2)))         # read x once, write mean + rstd


def ln_apply(x: Tensor, mod: Optional[Tensor], mod_sn: int, mean: Tensor, rstd: Tensor, y: Tensor):
    _dev(x, mod, mean, rstd, y)
    n, c = x.shape[0], x.shape[1]
    hw = x[0, 0].numel()
    _lib.check(_lib.load().sda_ln_apply(x.data_ptr(), n, c, hw, _ptr(mod), mod_sn, mean.data_ptr(), rstd.data_ptr(),
                                        y.data_ptr(), _stream()), 'sda_ln_apply')


def ln_bwd(gh: Tensor, x: Tensor, h: int, w: int, mod: Optional[Tensor], mod_sn: int, mean: Tensor, rstd: Tensor,
           unbiased: bool, pool, res: Optional[Tensor], gx: Tensor, out_amax: Optional[Tensor] = None):
    """pool: (pool_h, pool_w) -- the nearest-upsample factors whose backward (cell sums of gh) is fused in; (1, 1) = none.
    out_amax (device scalar, optional): receives max |gx| -- the input scale of an f16 x 2 convolution that reads gx next."""
    _dev(gh, x, mod, mean, rstd, res, gx, out_amax)
    n, c = x.shape[0], x.shape[1]

    def launch():
        if out_amax is None:
            _lib.check(_lib.load().sda_ln_bwd(gh.data_ptr(), x.data_ptr(), n, c, h, w, _ptr(mod), mod_sn, mean.data_ptr(),
                                              rstd.data_ptr(), int(unbiased), pool[0], pool[1], _ptr(res), gx.data_ptr(),
                                              _stream()), 'sda_ln_bwd')
        else:
            _lib.check(_lib.load().sda_ln_bwd_amax(gh.data_ptr(), x.data_ptr(), n, c, h, w, _ptr(mod), mod_sn, mean.data_ptr(),
                                                   rstd.data_ptr(), int(unbiased), pool[0], pool[1], _ptr(res), gx.data_ptr(),
                                                   out_amax.data_ptr(), _stream()), 'sda_ln_bwd_amax')
    # read gh (at the pooled resolution), x, res; write gx; + the statistics
    _bracketed(launch, lambda: ('ln_bwd', None, 4.0 * n * h * w * (c * (pool[0] * pool[1] + 2 + (1 if res is not None else 0)) + 2)))


# ------------------------------------------------------------------------------------------ time embedding

def time_embed(t: Tensor, freqs: Tensor, w0: Tensor, b0: Tensor, w2: Tensor, b2: Tensor) -> Tensor:
    _dev(t, freqs, w0, b0, w2, b2)
    nt = t.numel()
    e = w2.shape[0]
    emb = torch.empty(nt, e, device=t.device, dtype=torch.float32)
    _lib.check(_lib.load().sda_time_embed(t.data_ptr(), nt, freqs.data_ptr(), freqs.numel(), w0.data_ptr(), b0.data_ptr(),
                                          w0.shape[0], w2.data_ptr(), b2.data_ptr(), e, emb.data_ptr(), _stream()),
               'sda_time_embed')
    return emb


def linear_small(x: Tensor, w: Tensor, b: Tensor) -> Tensor:
    _dev(x, w, b)
    rows, in_f = x.shape
    out_f = w.shape[0]
    y = torch.empty(rows, out_f, device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().sda_linear_small(x.data_ptr(), rows, in_f, w.data_ptr(), b.data_ptr(), out_f, y.data_ptr(),
                                            _stream()), 'sda_linear_small')
    return y


# ------------------------------------------------------------------------------------------ ResMLP pieces

def linear(x: Tensor, w: Tensor, b: Optional[Tensor], *, trans_w: bool = False, act_in: int = 0, act_out: int = 0,
           dact_z: Optional[Tensor] = None, act_d: int = 0, res: Optional[Tensor] = None) -> Tensor:
    """x: (rows, in) contiguous.  trans_w=False: w is torch's [out][in] (forward);  True: w is [in][out] (gx = gy @ W)."""
    _dev(x, w, b, dact_z, res)
    rows, in_f = x.shape
    out_f = w.shape[1] if trans_w else w.shape[0]
    assert (w.shape[0] if trans_w else w.shape[1]) == in_f
    y = torch.empty(rows, out_f, device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().sda_linear(x.data_ptr(), rows, in_f, w.data_ptr(), _ptr(b), out_f, int(trans_w), act_in,
                                      act_out, _ptr(dact_z), act_d, _ptr(res), y.data_ptr(), _stream()), 'sda_linear')
    return y


def row_ln(x: Tensor, eps: float, unbiased: bool, y: Tensor, mean: Optional[Tensor] = None,
           rstd: Optional[Tensor] = None):
    _dev(x, y, mean, rstd)
    rows, f = x.shape
    _lib.check(_lib.load().sda_row_ln(x.data_ptr(), rows, f, eps, int(unbiased), y.data_ptr(), _ptr(mean), _ptr(rstd),
                                      _stream()), 'sda_row_ln')


def row_ln_bwd(gh: Tensor, x: Tensor, mean: Tensor, rstd: Tensor, unbiased: bool, res: Optional[Tensor], gx: Tensor):
    _dev(gh, x, mean, rstd, res, gx)
    rows, f = x.shape
    _lib.check(_lib.load().sda_row_ln_bwd(gh.data_ptr(), x.data_ptr(), rows, f, mean.data_ptr(), rstd.data_ptr(),
                                          int(unbiased), _ptr(res), gx.data_ptr(), _stream()), 'sda_row_ln_bwd')


def mlp_launch(d: '_lib.MlpDesc', backward: bool):
    """A whole ResMLP in one launch (csrc/mlp1d.hip), forward or input VJP; see include/sda_hip.h."""
    lib = _lib.load()
    fn, name = (lib.sda_mlp_bwd, 'sda_mlp_bwd') if backward else (lib.sda_mlp_fwd, 'sda_mlp_fwd')
    _mlp_bracket('mlp_bwd' if backward else 'mlp_fwd', d, lambda: _lib.check(fn(ctypes.byref(d), _stream()), name))


def _mlp_bracket(tag: str, d: '_lib.MlpDesc', launch):
    """Every GEMM of the ResMLP once over all rows."""
    _bracketed(launch, lambda: (tag, 2.0 * d.rows * sum(d.in_f[g] * d.out_f[g] for g in range(d.ngemm)), None))


def mlp_launch_win(d: '_lib.MlpDesc', w: '_lib.MlpWin', backward: bool):
    """One half of a fused guided evaluation of a local score network (sda_mlp_fwd_win / sda_mlp_bwd_win; sda_amd/fused1d.py)."""
    lib = _lib.load()
    fn, name = (lib.sda_mlp_bwd_win, 'sda_mlp_bwd_win') if backward else (lib.sda_mlp_fwd_win, 'sda_mlp_fwd_win')
    _mlp_bracket('mlp_bwd' if backward else 'mlp_fwd', d, lambda: _lib.check(fn(ctypes.byref(d), ctypes.byref(w), _stream()), name))


def mlp_bwd_train(d: '_lib.MlpTrainDesc'):
    """The input VJP of a whole ResMLP that also stores the cotangent at every GEMM's output (sda_mlp_bwd_train, csrc/mlp_train.hip)."""
    lib = _lib.load()
    _mlp_bracket('mlp_bwd', d.mlp, lambda: _lib.check(lib.sda_mlp_bwd_train(ctypes.byref(d), _stream()), 'sda_mlp_bwd_train'))


def adamw_step(d: '_lib.AdamWDesc') -> None:
    """One multi-tensor AdamW launch with the pack epilogue (sda_adamw_step, csrc/optim.hip; sda_amd.training.AdamW)."""
    _lib.check(_lib.load().sda_adamw_step(ctypes.byref(d), _stream()), 'sda_adamw_step')


def adamw_step_dev(d: '_lib.AdamWDesc', table: Tensor, irow: Tensor) -> None:
    """The same launch with {decay, step_size, rsqrt_bc2} = row ``irow[0]`` of the fp32 device ``table`` [rows][3] (sda_adamw_step_dev:
    hipGraph-replayable; sda_amd.training.GraphedStep).  The caller keeps ``irow`` (a device int64 scalar) inside the table."""
    if not (table.is_cuda and table.dtype == torch.float32 and table.is_contiguous() and table.dim() == 2 and table.shape[1] == 3):
        raise _lib.SdaHipError('adamw_step_dev: table is a contiguous fp32 device tensor [rows][3]')
    if not (irow.is_cuda and irow.dtype == torch.int64 and irow.numel() == 1):
        raise _lib.SdaHipError('adamw_step_dev: irow is a device int64 scalar')
    _lib.check(_lib.load().sda_adamw_step_dev(ctypes.byref(d), table.data_ptr(), irow.data_ptr(), _stream()), 'sda_adamw_step_dev')


def loss_perturb(x: Tensor, seed: int, row0: int, alpha_kind: int, eta: float, k: float, sigma_kind: int, step: int = 0,
                 step_dev: Optional[Tensor] = None):
    """x (rows, ...) -> (t (rows,), eps, xt) of the keyed denoising loss in one launch (sda_loss_perturb, csrc/train_loss.hip):
    eps[b] = row ``row0 + b`` of ``randn_rows(seed, draw = 2 s)``, t[b] a uniform in (0, 1) from draw ``2 s + 1`` of the same generator,
    xt = mu(t) x + sigma(t) eps with ``vp_schedule``'s mu and sigma.  s = ``step_dev[0]`` (a device int64 scalar: graph replay) or ``step``."""
    _dev(x)
    if step_dev is not None and (not step_dev.is_cuda or step_dev.dtype != torch.int64 or step_dev.numel() != 1):
        raise _lib.SdaHipError('step_dev must be a device int64 scalar')
    x = x.contiguous()
    rows = x.shape[0] if x.dim() else 0
    if rows < 1 or x.numel() == 0:
        raise _lib.SdaHipError('loss_perturb: x has at least one row and one element per row')
    t = torch.empty(rows, device=x.device, dtype=torch.float32)
    eps, xt = torch.empty_like(x), torch.empty_like(x)
    _lib.check(_lib.load().sda_loss_perturb(x.data_ptr(), rows, x.numel() // rows, seed & 0xffffffffffffffff, row0, step, _ptr(step_dev),
                                            alpha_kind, eta, k, sigma_kind, t.data_ptr(), eps.data_ptr(), xt.data_ptr(), _stream()),
               'sda_loss_perturb')
    return t, eps, xt


def loss_mse_plan(numel: int):
    """(workgroups of stage 1 = floats of the work buffer, longest chain of additions a term passes through) of ``loss_mse`` on ``numel``
    elements (sda_loss_mse_plan)."""
    blocks, chain = ctypes.c_int(0), ctypes.c_int(0)
    floats = _lib.load().sda_loss_mse_plan(numel, ctypes.byref(blocks), ctypes.byref(chain))
    _lib.check(int(min(floats, 0)), 'sda_loss_mse_plan')
    return blocks.value, chain.value


def loss_mse(out: Tensor, eps: Tensor, with_g: bool = True):
    """(0-dim mean((out - eps)^2), g = (2 / numel) (out - eps) or None): two ordered launches, bitwise reproducible (sda_loss_mse,
    csrc/train_loss.hip).  ``out`` and ``eps`` are contiguous and of one shape."""
    _dev(out, eps)
    if out.shape != eps.shape or not out.is_contiguous() or not eps.is_contiguous():
        raise _lib.SdaHipError('loss_mse: out and eps are contiguous tensors of one shape')
    blocks, _chain = loss_mse_plan(out.numel())
    loss = torch.empty((), device=out.device, dtype=torch.float32)
    work = torch.empty(blocks, device=out.device, dtype=torch.float32)
    g = torch.empty_like(out) if with_g else None
    _lib.check(_lib.load().sda_loss_mse(out.data_ptr(), eps.data_ptr(), out.numel(), loss.data_ptr(), _ptr(g), work.data_ptr(), _stream()),
               'sda_loss_mse')
    return loss, g


def window_batch_plan(n: int, length: int, window: int, batch: int, seed: int, step: int, rows: int):
    """Host only: (src_row, start), two int64 CPU tensors of ``rows`` entries -- the trajectory and first frame of every row of global
    batch ``step`` of ``window_batch`` (sda_window_batch_plan, csrc/dataset.hip: the kernel's own index functions).  Needs no GPU."""
    src_row, start = torch.empty(max(rows, 0), dtype=torch.int64), torch.empty(max(rows, 0), dtype=torch.int64)
    p64 = ctypes.POINTER(ctypes.c_int64)
    _lib.check(_lib.load().sda_window_batch_plan(n, length, window, batch, seed & 0xffffffffffffffff, step, rows,
                                                 ctypes.cast(src_row.data_ptr(), p64), ctypes.cast(start.data_ptr(), p64)),
               'sda_window_batch_plan')
    return src_row, start


def window_batch(data: Tensor, window: int, batch: int, rows: int, seed: int, step: int = 0, step_dev: Optional[Tensor] = None,
                 out: Optional[Tensor] = None) -> Tensor:
    """data (N, L, *frame) -> (rows, window, *frame): the rows of global batch s of the shuffled, randomly windowed dataset in one launch
    (sda_window_batch, csrc/dataset.hip).  Row b is ``data[n_b, start_b:start_b + window]`` with ``(n_b, start_b)`` of
    ``window_batch_plan``; s = ``step_dev[0]`` (a device int64 scalar the launch only reads: graph replay) or ``step``.  ``rows <= batch``
    (the epoch's short last batch).  ``out``: a contiguous fp32 device tensor of rows * window * frame elements to fill."""
    _dev(data, out)
    if step_dev is not None and (not step_dev.is_cuda or step_dev.dtype != torch.int64 or step_dev.numel() != 1):
        raise _lib.SdaHipError('step_dev must be a device int64 scalar')
    if data.dim() < 2 or not data.is_contiguous() or data.numel() == 0:
        raise _lib.SdaHipError('window_batch: data is a contiguous tensor (N, L, *frame) with at least one element')
    n, length = data.shape[:2]
    f = data.numel() // (n * length)
    if out is None:
        out = torch.empty((max(rows, 0), max(window, 0)) + tuple(data.shape[2:]), device=data.device, dtype=torch.float32)
    elif not out.is_contiguous() or out.numel() != rows * window * f or out.device != data.device:
        raise _lib.SdaHipError('window_batch: out is a contiguous tensor of rows * window * frame elements on the device of data')
    _lib.check(_lib.load().sda_window_batch(data.data_ptr(), n, length, f, window, batch, rows, seed & 0xffffffffffffffff, step,
                                            _ptr(step_dev), out.data_ptr(), _stream()), 'sda_window_batch')
    return out


def mlp_wgrad_work_floats(d: '_lib.MlpWgradDesc') -> int:
    """Floats of the ``work`` buffer sda_mlp_wgrad needs for this descriptor (``d.work`` is not read)."""
    floats = _lib.load().sda_mlp_wgrad_work_floats(ctypes.byref(d))
    _lib.check(int(min(floats, 0)), 'sda_mlp_wgrad_work_floats')
    return int(floats)


def mlp_wgrad(d: '_lib.MlpWgradDesc') -> None:
    """dw[g] / db[g] (+)= the weight and bias gradients of every GEMM of a ResMLP: one launch + one slab reduction (sda_mlp_wgrad,
    csrc/mlp_train.hip).  ``d.work`` holds mlp_wgrad_work_floats(d) floats."""
    lib = _lib.load()
    _bracketed(lambda: _lib.check(lib.sda_mlp_wgrad(ctypes.byref(d), _stream()), 'sda_mlp_wgrad'),
               lambda: ('wgrad', 2.0 * d.rows * sum((d.in_f[g] + 1) * d.out_f[g] for g in range(d.ngemm)), None))


def mc_finish(eps: Tensor, ghat: Tensor, gwin: Tensor, b: int, nw: int, k: int, c: int, cx0: float, cx1: float, coef_ptr: int, mode: int,
              out: Optional[Tensor], xs: Optional[Tensor], step_coef_ptr: int, partial: Optional[Tensor]):
    _dev(eps, ghat, gwin, out, xs, partial)
    _lib.check(_lib.load().sda_mc_finish(eps.data_ptr(), ghat.data_ptr(), gwin.data_ptr(), b, nw, k, c, cx0, cx1, coef_ptr, mode,
                                         _ptr(out), _ptr(xs), step_coef_ptr, _ptr(partial), _stream()), 'sda_mc_finish')


# ------------------------------------------------------------------------------------------ fold / unfold adjoints

def fold(s: Tensor, b: int, nw: int, k: int, c: int, hw: int, out: Tensor):
    _dev(s, out)
    _lib.check(_lib.load().sda_fold(s.data_ptr(), b, nw, k, c, hw, out.data_ptr(), _stream()), 'sda_fold')


def fold_adjoint(g_out: Tensor, b: int, nw: int, k: int, c: int, hw: int, g_s: Tensor):
    _dev(g_out, g_s)
    _lib.check(_lib.load().sda_fold_adjoint(g_out.data_ptr(), b, nw, k, c, hw, g_s.data_ptr(), _stream()),
               'sda_fold_adjoint')


def unfold_adjoint(g_win: Tensor, b: int, nw: int, k: int, c: int, hw: int, win_c_total: int, g_x: Tensor):
    _dev(g_win, g_x)
    _lib.check(_lib.load().sda_unfold_adjoint(g_win.data_ptr(), b, nw, k, c, hw, win_c_total, g_x.data_ptr(), _stream()),
               'sda_unfold_adjoint')


# ------------------------------------------------------------------------------------------ PC updates / guidance

def pc_predict(x: Tensor, eps: Tensor, r: float, c1: float, coef_dev: Optional[Tensor] = None):
    _dev(x, eps, coef_dev)
    _lib.check(_lib.load().sda_pc_predict(x.data_ptr(), eps.data_ptr(), x.numel(), r, c1, _ptr(coef_dev), _stream()),
               'sda_pc_predict')


SUMSQ_CHUNKS = 64


def _check_partial(partial: Tensor, b: int):
    if partial.numel() < b * SUMSQ_CHUNKS or not partial.is_contiguous():
        raise _lib.SdaHipError(f'partial-sum buffer needs {b} x {SUMSQ_CHUNKS} contiguous floats, got {tuple(partial.shape)}')


def sumsq_chunks(per_sample: int) -> int:
    """Workgroups per sample of the two-stage sum of squares: one per 4096 elements, at most SUMSQ_CHUNKS.  (A fixed 64 gave the Lorenz
    trajectories -- 195 elements -- 64 workgroups of three elements each: 32 us per correction at eval.py's batch.)"""
    return max(1, min(SUMSQ_CHUNKS, per_sample // 4096))


def sumsq_partial(eps: Tensor, b: int, partial: Tensor) -> int:
    """partial[b][nchunk] <- per-chunk sums of eps^2; returns nchunk (pass it to pc_correct)."""
    _dev(eps, partial)
    _check_partial(partial, b)
    per = eps.numel() // b
    nchunk = sumsq_chunks(per)
    _lib.check(_lib.load().sda_sumsq_partial(eps.data_ptr(), b, per, partial.data_ptr(), nchunk, _stream()),
               'sda_sumsq_partial')
    return nchunk


def pc_correct(x: Tensor, eps: Tensor, z: Tensor, b: int, partial: Tensor, tau: float, sigma: float,
               coef_dev: Optional[Tensor] = None, nchunk: Optional[int] = None):
    _dev(x, eps, z, partial, coef_dev)
    if nchunk is None:
        nchunk = sumsq_chunks(x.numel() // b)             # (what sumsq_partial wrote for this sample size)
    if partial.numel() < b * nchunk or not partial.is_contiguous():
        raise _lib.SdaHipError(f'partial-sum buffer needs {b} x {nchunk} contiguous floats, got {tuple(partial.shape)}')
    per = x.numel() // b
    _lib.check(_lib.load().sda_pc_correct(x.data_ptr(), eps.data_ptr(), z.data_ptr(), b, per, partial.data_ptr(),
                                          nchunk, tau, sigma, _ptr(coef_dev), _stream()), 'sda_pc_correct')


#: rows sda_pc_correct_keyed takes (its batch axis is grid.y; csrc/step1d.hip returns SDA_E_BADARG above)
PC_KEYED_MAX_ROWS = 65535


def pc_correct_keyed(x: Tensor, eps: Tensor, b: int, partial: Tensor, nchunk: int, tau: float, coef_dev: Tensor, seed: int, row0: int,
                     draw_dev: Tensor, draw_mul: int, draw_add: int):
    """The corrector update with its row-keyed noise generated in the kernel (the z of randn_rows(seed, row0, draw_dev * mul + add))."""
    _dev(x, eps, partial, coef_dev)
    if partial.numel() < b * nchunk or not partial.is_contiguous():
        raise _lib.SdaHipError(f'partial-sum buffer needs {b} x {nchunk} contiguous floats, got {tuple(partial.shape)}')
    if not draw_dev.is_cuda or draw_dev.dtype != torch.int64:
        raise _lib.SdaHipError('draw_dev must be a device int64 scalar')
    per = x.numel() // b
    _lib.check(_lib.load().sda_pc_correct_keyed(x.data_ptr(), eps.data_ptr(), b, per, partial.data_ptr(), nchunk, tau, 0.0,
                                                coef_dev.data_ptr(), seed & 0xffffffffffffffff, row0, draw_dev.data_ptr(), draw_mul,
                                                draw_add, _stream()), 'sda_pc_correct_keyed')


def randn_rows(out: Tensor, seed: int, row0: int, draw: int = 0, draw_dev: Optional[Tensor] = None, draw_mul: int = 1,
               draw_add: int = 0):
    """out (rows, ...) <- N(0, 1) draws keyed per row: out[r] depends on (seed, row0 + r, draw) only.  With ``draw_dev`` (a
    device int64 scalar) the draw index is ``draw_dev * draw_mul + draw_add``, read on the device (graph replay)."""
    _dev(out)
    if not out.is_contiguous():
        raise _lib.SdaHipError('randn_rows writes a contiguous tensor')
    if draw_dev is not None and (not draw_dev.is_cuda or draw_dev.dtype != torch.int64):
        raise _lib.SdaHipError('draw_dev must be a device int64 scalar')
    rows = out.shape[0]
    if out.numel() == 0:                    # an empty shard (batch < world size): nothing to draw
        return out
    _lib.check(_lib.load().sda_randn_rows(out.data_ptr(), rows, out.numel() // max(rows, 1), seed & 0xffffffffffffffff, row0,
                                          draw, _ptr(draw_dev), draw_mul, draw_add, _stream()), 'sda_randn_rows')
    return out


def vp_schedule(t: Tensor, alpha_kind: int, eta: float, k: float, sigma_kind: int) -> Tensor:
    """Device scalar t -> device pair {mu(t), sigma(t)} in one launch."""
    _dev(t)
    out = torch.empty(2, device=t.device, dtype=torch.float32)
    _lib.check(_lib.load().sda_vp_schedule(t.data_ptr(), alpha_kind, eta, k, sigma_kind, out.data_ptr(), _stream()),
               'sda_vp_schedule')
    return out


def _adjacent_pair(mu, sigma):
    """mu, sigma that are elements 0 and 1 of one fp32 device buffer (what vp_schedule returns) already form the pair."""
    if isinstance(mu, Tensor) and isinstance(sigma, Tensor) and mu.is_cuda and mu.dtype == sigma.dtype == torch.float32 \
            and mu.numel() == sigma.numel() == 1 and sigma.data_ptr() == mu.data_ptr() + 4 \
            and mu.untyped_storage().data_ptr() == sigma.untyped_storage().data_ptr():
        return mu.as_strided((2,), (1,))
    return None


def _coef(mu, sigma):
    """python floats travel by value; 0-dim device tensors travel as a device {mu, sigma} pair (no host sync)."""
    if isinstance(mu, Tensor) or isinstance(sigma, Tensor):
        pair = _adjacent_pair(mu, sigma)
        if pair is not None:
            return 0.0, 0.0, pair
        dev = mu.device if isinstance(mu, Tensor) else sigma.device
        pair = torch.stack([torch.as_tensor(mu, dtype=torch.float32, device=dev).reshape(()),
                            torch.as_tensor(sigma, dtype=torch.float32, device=dev).reshape(())])
        return 0.0, 0.0, pair
    return float(mu), float(sigma), None


def denoise(x: Tensor, eps: Tensor, mu, sigma, xhat: Tensor):
    _dev(x, eps, xhat)
    m, s, pair = _coef(mu, sigma)
    _lib.check(_lib.load().sda_denoise(x.data_ptr(), eps.data_ptr(), x.numel(), m, s, _ptr(pair), xhat.data_ptr(),
                                       _stream()), 'sda_denoise')


def guided_combine(eps: Tensor, ghat: Tensor, vjp: Optional[Tensor], mu, sigma, out: Tensor):
    _dev(eps, ghat, vjp, out)
    m, s, pair = _coef(mu, sigma)
    _lib.check(_lib.load().sda_guided_combine(eps.data_ptr(), ghat.data_ptr(), _ptr(vjp), eps.numel(), m, s, _ptr(pair),
                                              out.data_ptr(), _stream()), 'sda_guided_combine')


def gauss_cotangent(y: Tensor, ax: Tensor, std: float, gamma: float, mu, sigma) -> Tensor:
    """(y - ax) / (std^2 + gamma (sigma/mu)^2) for scalar std / gamma; y broadcasts over ax's leading axis."""
    _dev(y, ax)
    y, ax = y.contiguous(), ax.contiguous()
    out = torch.empty_like(ax)
    m, s, pair = _coef(mu, sigma)
    _lib.check(_lib.load().sda_gauss_cotangent(y.data_ptr(), y.numel(), ax.data_ptr(), ax.numel(), float(std), float(gamma), m, s,
                                               _ptr(pair), out.data_ptr(), _stream()), 'sda_gauss_cotangent')
    return out


# ---------------------------------------------------------------------------------------------- evaluation metrics
def pairwise_dist(x: Tensor, y: Tensor, squared: bool) -> Tensor:
    """x: (m, d), y: (n, d) -> (m, n) Euclidean distances (or their squares)."""
    _dev(x, y)
    x, y = x.contiguous(), y.contiguous()
    if x.dim() != 2 or y.dim() != 2 or x.shape[1] != y.shape[1]:
        raise _lib.SdaHipError(f'pairwise_dist: incompatible shapes {tuple(x.shape)} / {tuple(y.shape)}')
    out = torch.empty(x.shape[0], y.shape[0], device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().sda_pairwise_dist(x.data_ptr(), x.shape[0], y.data_ptr(), y.shape[0], x.shape[1],
                                             0 if squared else 1, out.data_ptr(), _stream()), 'sda_pairwise_dist')
    return out


def mmd_kernel_sum(d2: Tensor) -> Tensor:
    """sum_ij sum_sigma exp(-d2_ij / sigma) as a 0-dim float64 device tensor."""
    _dev(d2)
    d2 = d2.contiguous()
    nblocks = int(min(1024, max(1, (d2.numel() + 255) // 256)))
    partial = torch.empty(nblocks, device=d2.device, dtype=torch.float64)
    _lib.check(_lib.load().sda_mmd_kernel_sums(d2.data_ptr(), d2.numel(), partial.data_ptr(), nblocks, _stream()),
               'sda_mmd_kernel_sums')
    return partial.sum()


def transport_cost(cost: Tensor) -> float:
    """Host optimal-transport solve with uniform marginals of an (m, n) fp32 host cost matrix: min_P <P, cost>."""
    if cost.is_cuda or cost.dtype != torch.float32 or cost.dim() != 2:
        raise _lib.SdaHipError('transport_cost expects an fp32 host matrix')
    cost = cost.contiguous()
    total = ctypes.c_double(0.0)
    _lib.check(_lib.load().sda_transport_cost(cost.data_ptr(), cost.shape[0], cost.shape[1], ctypes.addressof(total)),
               'sda_transport_cost')
    return total.value


def assignment_cost(cost: Tensor):
    """Host linear-assignment solve of a square cost matrix (CPU tensor): (minimum total cost, column of each row)."""
    if cost.is_cuda or cost.dtype != torch.float32 or cost.dim() != 2 or cost.shape[0] != cost.shape[1]:
        raise _lib.SdaHipError('assignment_cost expects a square fp32 host matrix')
    cost = cost.contiguous()
    n = cost.shape[0]
    total = ctypes.c_double(0.0)
    cols = torch.empty(n, dtype=torch.int32)
    _lib.check(_lib.load().sda_assignment_cost(cost.data_ptr(), n, ctypes.addressof(total), cols.data_ptr()),
               'sda_assignment_cost')
    return total.value, cols


#: largest n sda_assignment_auction serves (SDA_AUCTION_MAX_N: its state lives in LDS)
AUCTION_MAX_N = 4096
#: per-problem status words of sda_assignment_auction (include/sda_hip.h)
AUCTION_CONVERGED, AUCTION_NOT_CONVERGED, AUCTION_BADARG = 0, 1, -1
#: default bid budget = min(AUCTION_BIDS_PER_ROW * n, AUCTION_BID_CAP): 8 x the largest bids / n the host replay showed, capped
#: where a launch that spends the whole budget would pass about a second at n = 4096
AUCTION_BIDS_PER_ROW = 8 * 161
AUCTION_BID_CAP = 160 * 4096


def auction_default_budget(n: int) -> int:
    return min(AUCTION_BIDS_PER_ROW * n, AUCTION_BID_CAP)

AuctionResult = collections.namedtuple('AuctionResult', 'total gap eps_final bids status col_of_row record')


def auction_record(record: Tensor, batch: int):
    """Views of the five per-problem words in an AuctionResult.record (device or host copy): total, gap, eps_final (float64),
    bids (int64), status (int32)."""
    w = 8 * batch
    return (record[0:w].view(torch.float64), record[w:2 * w].view(torch.float64), record[2 * w:3 * w].view(torch.float64),
            record[3 * w:4 * w].view(torch.int64), record[4 * w:4 * w + 4 * batch].view(torch.int32))


def assignment_auction(cost: Tensor, eps_rel: float = 1e-7, bid_budget=None) -> AuctionResult:
    """Device linear-assignment solve (epsilon-scaling auction, ``sda_assignment_auction``) of an fp32 device tensor (n, n) or
    (b, n, n), n <= AUCTION_MAX_N.  Returns device tensors: total, gap, eps_final (float64), bids (int64), status (int32) -- 0-dim
    for an (n, n) input, (b,) otherwise -- and col_of_row (int32, (n,) or (b, n)); ``record`` is the one byte buffer the five
    words live in (one copy brings them all to the host).  total - optimum <= gap <= n eps_final where status is
    AUCTION_CONVERGED; AUCTION_NOT_CONVERGED: ``bid_budget`` (default ``auction_default_budget(n)``) ran out; AUCTION_BADARG: NaN /
    inf costs.  Nothing synchronises."""
    _dev(cost)
    if cost.dtype != torch.float32 or cost.dim() not in (2, 3) or cost.shape[-1] != cost.shape[-2] or cost.shape[-1] < 1:
        raise _lib.SdaHipError('assignment_auction expects a square fp32 device matrix (n, n) or a batch (b, n, n)')
    single = cost.dim() == 2
    cost = cost.contiguous()
    n = cost.shape[-1]
    batch = 1 if single else cost.shape[0]
    if batch < 1:
        raise _lib.SdaHipError('assignment_auction: empty batch')
    if bid_budget is None:
        bid_budget = auction_default_budget(n)
    record = torch.empty(8 * 4 * batch + 8 * ((batch + 1) // 2), device=cost.device, dtype=torch.uint8)
    total, gap, eps_final, bids, status = auction_record(record, batch)
    cols = torch.empty(batch, n, device=cost.device, dtype=torch.int32)
    _lib.check(_lib.load().sda_assignment_auction(cost.data_ptr(), n, batch, float(eps_rel), int(bid_budget), total.data_ptr(),
                                                  gap.data_ptr(), eps_final.data_ptr(), bids.data_ptr(), status.data_ptr(),
                                                  cols.data_ptr(), _stream()), 'sda_assignment_auction')
    if single:
        total, gap, eps_final, bids, status, cols = total[0], gap[0], eps_final[0], bids[0], status[0], cols[0]
    return AuctionResult(total, gap, eps_final, bids, status, cols, record)


def clock_probe(device, ms: float = 2.0, blocks: int = 1024) -> dict:
    """The shader clock (GHz) the fp32 matrix-core stream sustains on ``device`` right now (``sda_clock_probe``): ``blocks``
    workgroups of four waves issue register-resident v_mfma_f32_16x16x4_f32 for about ``ms`` milliseconds and time themselves with
    the shader-clock and the 100 MHz counters.  Measurement support for bench.py; synchronises the device."""
    lib = _lib.load()
    out = torch.zeros(2 * blocks, device=device, dtype=torch.int64)
    sink = torch.zeros(1, device=device, dtype=torch.float32)
    # 8 MFMAs x 32 cycles per round and wave, one wave per SIMD per resident workgroup; `blocks` over 256 CUs run in waves of 256 x
    # (workgroups per CU): size the rounds so that the whole launch lasts ~ms at 2.4 GHz
    per_cu = max(1, -(-blocks // 256))
    iters = max(64, int(ms * 1e-3 * 2.4e9 / (8 * 32) / per_cu))
    with torch.cuda.device(device):
        for _ in range(2):                                  # (the first launch also pays the code upload)
            _lib.check(lib.sda_clock_probe(out.data_ptr(), blocks, sink.data_ptr(), iters, _stream()), 'sda_clock_probe')
        torch.cuda.synchronize(device)
    v = out.reshape(blocks, 2).double()
    ghz = (v[:, 0] / v[:, 1].clamp_min(1)) * 0.1
    return {'ghz': float(ghz.median()), 'ghz_min': float(ghz.min()), 'ghz_max': float(ghz.max()), 'blocks': blocks,
            'mfma_per_wave': iters * 8, 'instruction': 'v_mfma_f32_16x16x4_f32, register operands'}


# ---------------------------------------------------------------- Markov chains and the particle filter (csrc/chain.hip)
def chain_model(kind: str, d: int, dt: float, steps: int, params, noise_std: float = 0.0) -> '_lib.ChainModel':
    """`sda_chain_model`: h = dt / steps rounded to fp32 ONCE, as torch rounds the reference's python scalar."""
    m = _lib.ChainModel()
    m.kind, m.d, m.steps = _lib.CHAIN_KINDS[kind], int(d), int(steps)
    m.h = dt / steps
    for i, v in enumerate(params):
        m.p[i] = float(v)
    m.noise_std = float(noise_std)
    return m


def chain_obs(index, shift, scale, sigma: float, y: Tensor) -> '_lib.ChainObs':
    """`sda_chain_obs` for A(x) = (x[index] - shift) / scale observed as y (k,) with noise sigma."""
    _dev(y)
    o = _lib.ChainObs()
    o.k = len(index)
    if o.k > _lib.CHAIN_MAXOBS or y.numel() != o.k or not y.is_contiguous():
        raise _lib.SdaHipError(f'chain_obs: {o.k} observed components, y has {y.numel()} values')
    for i in range(o.k):
        o.idx[i], o.shift[i], o.scale[i] = int(index[i]), float(shift[i]), float(scale[i])
    o.sigma = float(sigma)
    o.y = y.data_ptr()
    o._keep = y
    return o


def _i32(t: Optional[Tensor], n: int, what: str):
    if t is None:
        return None
    if not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous() or t.numel() != n:
        raise _lib.SdaHipError(f'{what}: expected {n} contiguous int32 values on the device')
    return t.data_ptr()


def chain_advance(model, x: Tensor, out: Tensor, transitions: int, *, every: bool = False, out_st: int = 0, out_sp: Optional[int] = None,
                  anc: Optional[Tensor] = None, seed: int = 0, row0: int = 0, draw0: int = 0, obs=None,
                  logw: Optional[Tensor] = None, pmax: Optional[Tensor] = None) -> Tensor:
    """`transitions` transitions of x (m, d) in one launch.  `out` is a preallocated fp32 device tensor the caller addresses by
    strides (in floats): the last state at out[j * out_sp], or with every=True the state after transition t at
    out[t * out_st + j * out_sp].  The caller guarantees that those addresses lie inside `out`."""
    _dev(x, out, logw, pmax)
    m, d = x.shape
    if x.dim() != 2 or x.stride(1) != 1 or d != model.d:
        raise _lib.SdaHipError(f'chain_advance: states {tuple(x.shape)} (strides {x.stride()}) for a {model.d}-component chain')
    out_sp = d if out_sp is None else out_sp
    last = (transitions - 1) * out_st if every else 0
    if out_sp < d or (every and out_st < 0) or last + (m - 1) * out_sp + d > out.numel() or not out.is_contiguous():
        raise _lib.SdaHipError('chain_advance: the output strides leave the output tensor')
    a = _lib.ChainAdv()
    a.model = model
    a.x_in, a.in_sp, a.anc = x.data_ptr(), x.stride(0) if m > 1 else d, _i32(anc, m, 'chain_advance: anc')
    a.out, a.out_st, a.out_sp, a.every = out.data_ptr(), out_st, out_sp, int(every)
    a.m, a.transitions = m, transitions
    a.seed, a.row0, a.draw0 = seed & 0xffffffffffffffff, row0, draw0
    if obs is not None:
        nb = _lib.load().sda_bpf_logweights_blocks(m)
        if logw is None or pmax is None or logw.numel() < m or pmax.numel() < nb:
            raise _lib.SdaHipError('chain_advance: fused weights need logw (m,) and pmax (blocks,)')
        a.obs, a.logw, a.pmax = ctypes.pointer(obs), logw.data_ptr(), pmax.data_ptr()
    _lib.check(_lib.load().sda_chain_advance(ctypes.byref(a), _stream()), 'sda_chain_advance')
    return out


def chain_log_prob(model, x: Tensor) -> Tensor:
    """x (b, L, d) -> (b,) float64: sum_i log p(x_{i+1} | x_i) of the noisy chain."""
    _dev(x)
    if x.dim() != 3 or x.shape[2] != model.d or x.shape[1] < 2:
        raise _lib.SdaHipError(f'chain_log_prob: trajectories {tuple(x.shape)} for a {model.d}-component chain')
    if x.stride(2) != 1:
        x = x.contiguous()
    out = torch.empty(x.shape[0], device=x.device, dtype=torch.float64)
    _lib.check(_lib.load().sda_chain_log_prob(ctypes.byref(model), x.data_ptr(), x.shape[0], x.shape[1], x.stride(0), x.stride(1),
                                              out.data_ptr(), _stream()), 'sda_chain_log_prob')
    return out


def _rows(t: Tensor, shape, what: str) -> Tensor:
    """t as fp32 rows of the given shape whose components are contiguous (strides stay the caller's otherwise)."""
    _dev(t)
    if tuple(t.shape) != tuple(shape):
        raise _lib.SdaHipError(f'{what}: shape {tuple(t.shape)}, expected {tuple(shape)}')
    return t if t.stride(-1) == 1 else t.contiguous()


def chain_advance_vjp(model, x_in: Tensor, states: Optional[Tensor], g: Tensor, transitions: int, every: bool) -> Tensor:
    """The cotangent (m, d) of x_in under `chain_advance(model, x_in, .., transitions, every=every)`, one launch.  `states`
    (>= transitions - 1, m, d): the states after each transition as an every=True forward wrote them (with its noise, if any); None is
    allowed for one transition.  g: (transitions, m, d) with every=True, the cotangent of every kept state, else (m, d)."""
    if x_in.dim() != 2 or x_in.shape[1] != model.d or transitions < 1:
        raise _lib.SdaHipError(f'chain_advance_vjp: states {tuple(x_in.shape)} for a {model.d}-component chain, {transitions} transitions')
    m, d = x_in.shape
    x_in = _rows(x_in, (m, d), 'chain_advance_vjp: x_in')
    g = _rows(g, (transitions, m, d) if every else (m, d), 'chain_advance_vjp: g')
    a = _lib.ChainVjp()
    a.model = model
    a.x_in, a.in_sp = x_in.data_ptr(), x_in.stride(0) if m > 1 else d
    if transitions > 1:
        if states is None or states.dim() != 3 or states.shape[0] < transitions - 1:
            raise _lib.SdaHipError(f'chain_advance_vjp: {transitions} transitions need the {transitions - 1} states between them')
        states = _rows(states, (states.shape[0], m, d), 'chain_advance_vjp: states')
        a.states, a.st_st, a.st_sp = states.data_ptr(), states.stride(0), states.stride(1) if m > 1 else d
    a.g, a.g_sp = g.data_ptr(), g.stride(-2) if m > 1 else d
    a.g_st = g.stride(0) if every and transitions > 1 else 0
    a.every, a.m, a.transitions = int(every), m, transitions
    gx = torch.empty(m, d, device=x_in.device, dtype=torch.float32)
    a.gx, a.gx_sp = gx.data_ptr(), d
    _lib.check(_lib.load().sda_chain_advance_vjp(ctypes.byref(a), _stream()), 'sda_chain_advance_vjp')
    return gx


def chain_log_prob_grad(model, x: Tensor):
    """x (b, L, d) -> (value (b,) float64 -- bitwise `chain_log_prob` -- and its gradient (b, L, d) fp32), one launch.  The
    gradient is that of each value with cotangent 1; a caller with another cotangent scales it."""
    _dev(x)
    if x.dim() != 3 or x.shape[2] != model.d or x.shape[1] < 2:
        raise _lib.SdaHipError(f'chain_log_prob_grad: trajectories {tuple(x.shape)} for a {model.d}-component chain')
    if x.stride(2) != 1:
        x = x.contiguous()
    out = torch.empty(x.shape[0], device=x.device, dtype=torch.float64)
    grad = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().sda_chain_log_prob_grad(ctypes.byref(model), x.data_ptr(), x.shape[0], x.shape[1], x.stride(0), x.stride(1),
                                                   out.data_ptr(), grad.data_ptr(), _stream()), 'sda_chain_log_prob_grad')
    return out, grad


def bpf_logweights(x: Tensor, obs):
    """x (m, d) -> (logw (m,), pmax (blocks,)): affine-select Gaussian log-weights and the per-workgroup maxima."""
    _dev(x)
    if x.dim() != 2 or x.stride(1) != 1:
        raise _lib.SdaHipError(f'bpf_logweights: states {tuple(x.shape)} (strides {x.stride()})')
    m, d = x.shape
    lib = _lib.load()
    logw = torch.empty(m, device=x.device, dtype=torch.float32)
    pmax = torch.empty(lib.sda_bpf_logweights_blocks(m), device=x.device, dtype=torch.float32)
    _lib.check(lib.sda_bpf_logweights(x.data_ptr(), m, x.stride(0) if m > 1 else d, d, ctypes.byref(obs), logw.data_ptr(),
                                      pmax.data_ptr(), _stream()), 'sda_bpf_logweights')
    return logw, pmax


def bpf_cdf(logw: Tensor, pmax: Optional[Tensor] = None, *, w: Optional[Tensor] = None, cdf: Optional[Tensor] = None,
            status: Optional[Tensor] = None, check: bool = True):
    """logw (m,) -> (w (m,) fp32 = exp(logw - max), cdf (m,) float64 inclusive prefix sums, status (1,) int32).  check=True reads
    the status (one synchronisation) and raises when no particle carries weight; a filter passes check=False and reads all its
    status words once at the end (`bpf_check`)."""
    _dev(logw, pmax)
    m = logw.numel()
    if not logw.is_contiguous() or (pmax is not None and not pmax.is_contiguous()):
        raise _lib.SdaHipError('bpf_cdf: contiguous vectors expected')
    w = torch.empty(m, device=logw.device, dtype=torch.float32) if w is None else w
    cdf = torch.empty(m, device=logw.device, dtype=torch.float64) if cdf is None else cdf
    status = torch.empty(1, device=logw.device, dtype=torch.int32) if status is None else status
    if w.numel() != m or cdf.numel() != m or cdf.dtype != torch.float64 or status.dtype != torch.int32 or status.numel() < 1:
        raise _lib.SdaHipError('bpf_cdf: w (m,) fp32, cdf (m,) float64 and status (1,) int32 expected')
    _lib.check(_lib.load().sda_bpf_cdf(logw.data_ptr(), m, _ptr(pmax), 0 if pmax is None else pmax.numel(), w.data_ptr(),
                                       cdf.data_ptr(), status.data_ptr(), _stream()), 'sda_bpf_cdf')
    if check:
        bpf_check(status)
    return w, cdf, status


def bpf_check(status: Tensor) -> None:
    """Raise if any observation left no particle with weight (every log-weight -inf, or a NaN): where the reference's
    torch.multinomial raises."""
    bad = status.nonzero().flatten().tolist()
    if bad:
        raise _lib.SdaHipError(f'particle filter: no particle carries weight at observation(s) {bad} (every log-weight is -inf, or '
                               f'one is NaN)')


def bpf_resample(cdf: Tensor, seed: int, obs_index: int, anc: Optional[Tensor] = None) -> Tensor:
    """cdf (m,) float64 -> (m,) int32 i.i.d. categorical ancestors (draw j of observation obs_index: csrc/philox.hpp)."""
    if not cdf.is_cuda or cdf.dtype != torch.float64 or not cdf.is_contiguous():
        raise _lib.SdaHipError('bpf_resample: a contiguous float64 device vector expected (there is no CPU fallback)')
    m = cdf.numel()
    anc = torch.empty(m, device=cdf.device, dtype=torch.int32) if anc is None else anc
    _lib.check(_lib.load().sda_bpf_resample(cdf.data_ptr(), m, seed & 0xffffffffffffffff, obs_index, _i32(anc, m, 'bpf_resample: anc'),
                                            _stream()), 'sda_bpf_resample')
    return anc


def bpf_traceback(S: Tensor, anc: Tensor, step: int) -> Tensor:
    """S (T + 1, m, d) un-resampled states, anc (N, m) int32, T = N step -> (m, T + 1, d) resampled trajectories."""
    _dev(S)
    if S.dim() != 3 or not S.is_contiguous() or anc.dim() != 2 or S.shape[0] != anc.shape[0] * step + 1 or anc.shape[1] != S.shape[1]:
        raise _lib.SdaHipError(f'bpf_traceback: states {tuple(S.shape)}, ancestors {tuple(anc.shape)}, step {step}')
    t1, m, d = S.shape
    out = torch.empty(m, t1, d, device=S.device, dtype=torch.float32)
    _lib.check(_lib.load().sda_bpf_traceback(S.data_ptr(), m * d, d, _i32(anc, anc.numel(), 'bpf_traceback: anc'), m, anc.shape[0], step, d,
                                             out.data_ptr(), _stream()), 'sda_bpf_traceback')
    return out


# ---------------------------------------------------------------- ensemble Kalman smoother (csrc/enks.hip)
def _enks_slabs(S: Tensor, what: str):
    _dev(S)
    if S.dim() != 3 or S.stride(2) != 1 or S.shape[1] < 2 or (S.stride(1) < S.shape[2]) or S.stride(0) < 0:
        raise _lib.SdaHipError(f'{what}: ensemble slabs {tuple(S.shape)} (strides {S.stride()}), expected (time, members, d) with '
                               f'contiguous components')


def _enks_scratch(t: Optional[Tensor], k: int, m: int, like: Tensor, what: str) -> Tensor:
    if t is None:
        return torch.empty(k, m, device=like.device, dtype=torch.float32)
    _dev(t)
    if tuple(t.shape) != (k, m) or not t.is_contiguous():
        raise _lib.SdaHipError(f'{what}: a contiguous ({k}, {m}) fp32 device tensor expected')
    return t


def enks_gain(S: Tensor, t: int, obs, *, inflation: float = 1.0, seed: int = 0, draw: int = 0, a: Optional[Tensor] = None,
              z: Optional[Tensor] = None, work: Optional[Tensor] = None, status: Optional[Tensor] = None):
    """Steps 2 - 4 of one analysis (include/sda_hip.h) on slab ``S[t]`` of the time-major ensemble S (time, members, d): the observed
    anomalies ``a`` and the solved perturbed innovations ``z``, both (k, members), and status (1,) int32 (1: the factorisation
    failed), one launch, nothing read back.  ``obs``: an ``ops.chain_obs`` carrying this observation's y.  S is only read."""
    _enks_slabs(S, 'enks_gain')
    if not 0 <= t < S.shape[0]:
        raise _lib.SdaHipError(f'enks_gain: slab {t} of {S.shape[0]}')
    m, d, k = S.shape[1], S.shape[2], obs.k
    a, z, work = (_enks_scratch(v, k, m, S, 'enks_gain') for v in (a, z, work))
    status = torch.zeros(1, device=S.device, dtype=torch.int32) if status is None else status
    if status.dtype != torch.int32 or status.numel() < 1 or not status.is_cuda:
        raise _lib.SdaHipError('enks_gain: status (1,) int32 on the device expected')
    x = S[t]
    _lib.check(_lib.load().sda_enks_gain(x.data_ptr(), m, S.stride(1), d, ctypes.byref(obs), float(inflation),
                                         seed & 0xffffffffffffffff, draw, a.data_ptr(), z.data_ptr(), work.data_ptr(),
                                         status.data_ptr(), _stream()), 'sda_enks_gain')
    return a, z, status


def enks_update(S: Tensor, lo: int, t: int, a: Tensor, z: Tensor, *, inflation: float = 1.0) -> Tensor:
    """Steps 1 and 5 of one analysis, in place on the slabs ``S[lo] .. S[t]`` (``S[t]`` the observed one), one launch."""
    _enks_slabs(S, 'enks_update')
    if not 0 <= lo <= t < S.shape[0]:
        raise _lib.SdaHipError(f'enks_update: window {lo} .. {t} of {S.shape[0]} slabs')
    m, d = S.shape[1], S.shape[2]
    _dev(a, z)
    k = a.shape[0] if a.dim() == 2 else 0
    if tuple(a.shape) != (k, m) or tuple(z.shape) != (k, m) or not a.is_contiguous() or not z.is_contiguous():
        raise _lib.SdaHipError(f'enks_update: a {tuple(a.shape)} and z {tuple(z.shape)}, expected contiguous (k, {m})')
    _lib.check(_lib.load().sda_enks_update(S[lo].data_ptr(), S.stride(0), S.stride(1), t - lo + 1, m, d, k, float(inflation),
                                           a.data_ptr(), z.data_ptr(), _stream()), 'sda_enks_update')
    return S


def enks_check(status: Tensor) -> None:
    """Raise if the innovation covariance of any analysis had no Cholesky factor (a pivot not positive and finite)."""
    bad = status.nonzero().flatten().tolist()
    if bad:
        raise _lib.SdaHipError(f'ensemble Kalman smoother: the innovation covariance is not positive definite at observation(s) {bad}')


# ---------------------------------------------------------------- its ensemble-space form (csrc/enks_wide.hip)
ENKW_MAX_M = 128


def _enkw_mk(t: Optional[Tensor], m: int, k: int, like: Tensor, what: str) -> Tensor:
    if t is None:
        return torch.empty(m, k, device=like.device, dtype=torch.float32)
    _dev(t)
    if tuple(t.shape) != (m, k) or not t.is_contiguous():
        raise _lib.SdaHipError(f'{what}: a contiguous ({m}, {k}) fp32 device tensor expected')
    return t


def _enkw_f64(t: Optional[Tensor], n: int, like: Tensor, what: str) -> Tensor:
    if t is None:
        return torch.empty(n, device=like.device, dtype=torch.float64)
    if not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous() or t.numel() < n:
        raise _lib.SdaHipError(f'{what}: at least {n} contiguous float64 values on the device expected')
    return t


def enkw_prepare(H: Tensor, y: Tensor, sigma: float, *, seed: int = 0, draw: int = 0, Y: Optional[Tensor] = None,
                 D: Optional[Tensor] = None, eps: Optional[Tensor] = None):
    """Step 2 of the ensemble-space analysis (include/sda_hip.h): H (members, k) observed values, y (k,) -> the anomalies ``Y``,
    the perturbed innovations ``D`` and the perturbations ``eps``, all (members, k), one launch."""
    _dev(H, y)
    if H.dim() != 2 or not H.is_contiguous() or H.shape[1] < 1 or y.numel() != H.shape[1] or not y.is_contiguous():
        raise _lib.SdaHipError(f'enkw_prepare: H {tuple(H.shape)} and y {tuple(y.shape)}, expected contiguous (members, k) and (k,)')
    m, k = H.shape
    Y, D, eps = (_enkw_mk(v, m, k, H, 'enkw_prepare') for v in (Y, D, eps))
    _lib.check(_lib.load().sda_enkw_prepare(H.data_ptr(), m, k, y.data_ptr(), float(sigma), seed & 0xffffffffffffffff, draw,
                                            Y.data_ptr(), D.data_ptr(), eps.data_ptr(), _stream()), 'sda_enkw_prepare')
    return Y, D, eps


def enkw_gram(Y: Tensor, D: Tensor, *, part: Optional[Tensor] = None) -> Tensor:
    """Step 3: the float64 partials of [Y Y^T | Y D^T], one (pad16(m), 2 pad16(m)) block per chunk of 512 observed values."""
    _dev(Y, D)
    if Y.dim() != 2 or Y.shape != D.shape or not Y.is_contiguous() or not D.is_contiguous() or Y.shape[1] < 1:
        raise _lib.SdaHipError(f'enkw_gram: Y {tuple(Y.shape)} and D {tuple(D.shape)}, expected contiguous (members, k)')
    m, k = Y.shape
    n = _lib.load().sda_enkw_gram_doubles(m, k)
    if n <= 0:
        _lib.check(-2, 'sda_enkw_gram')
    part = _enkw_f64(part, n, Y, 'enkw_gram: part')
    _lib.check(_lib.load().sda_enkw_gram(Y.data_ptr(), D.data_ptr(), m, k, part.data_ptr(), _stream()), 'sda_enkw_gram')
    return part


def enkw_solve(part: Tensor, m: int, k: int, sigma: float, *, W: Optional[Tensor] = None, status: Optional[Tensor] = None,
               work: Optional[Tensor] = None):
    """Step 4: ``W`` (m, m) fp32 and status (1,) int32 (1: no Cholesky factor, or a non-finite W; W is then zero) from the partials
    of ``enkw_gram(Y, D)`` with Y (m, k), one launch of one workgroup, nothing read back."""
    n = _lib.load().sda_enkw_gram_doubles(m, k)
    if n <= 0:
        _lib.check(-2, 'sda_enkw_solve')
    part = _enkw_f64(part, n, part, 'enkw_solve: part')
    work = _enkw_f64(work, m * m, part, 'enkw_solve: work')
    if W is None:
        W = torch.empty(m, m, device=part.device, dtype=torch.float32)
    _dev(W)
    if tuple(W.shape) != (m, m) or not W.is_contiguous():
        raise _lib.SdaHipError(f'enkw_solve: a contiguous ({m}, {m}) fp32 device tensor expected for W')
    status = torch.zeros(1, device=part.device, dtype=torch.int32) if status is None else status
    if status.dtype != torch.int32 or status.numel() < 1 or not status.is_cuda:
        raise _lib.SdaHipError('enkw_solve: status (1,) int32 on the device expected')
    _lib.check(_lib.load().sda_enkw_solve(part.data_ptr(), m, k, float(sigma), work.data_ptr(), W.data_ptr(), status.data_ptr(),
                                          _stream()), 'sda_enkw_solve')
    return W, status


def enkw_transform(S: Tensor, lo: int, t: int, W: Tensor) -> Tensor:
    """Step 5, in place on the slabs ``S[lo] .. S[t]`` of the time-major ensemble S (time, members, d), one launch."""
    _enks_slabs(S, 'enkw_transform')
    if not 0 <= lo <= t < S.shape[0]:
        raise _lib.SdaHipError(f'enkw_transform: window {lo} .. {t} of {S.shape[0]} slabs')
    m, d = S.shape[1], S.shape[2]
    _dev(W)
    if tuple(W.shape) != (m, m) or not W.is_contiguous():
        raise _lib.SdaHipError(f'enkw_transform: W {tuple(W.shape)}, expected contiguous ({m}, {m})')
    _lib.check(_lib.load().sda_enkw_transform(S[lo].data_ptr(), S.stride(0), S.stride(1), t - lo + 1, m, d, W.data_ptr(), 1.0, 0,
                                              _stream()), 'sda_enkw_transform')
    return S


def enkw_inflate(S: Tensor, t: int, inflation: float) -> Tensor:
    """Step 1, in place on slab ``S[t]`` (the transform launch in its inflation mode); ``inflation == 1`` launches nothing."""
    _enks_slabs(S, 'enkw_inflate')
    if not 0 <= t < S.shape[0]:
        raise _lib.SdaHipError(f'enkw_inflate: slab {t} of {S.shape[0]}')
    _lib.check(_lib.load().sda_enkw_transform(S[t].data_ptr(), S.stride(0), S.stride(1), 1, S.shape[1], S.shape[2], None,
                                              float(inflation), 1, _stream()), 'sda_enkw_transform')
    return S


# ---------------------------------------------------------------- its domain-localised form (csrc/enks_local.hip)
def gaspari_cohn(z):
    """The Gaspari-Cohn fifth-order function of a float64 numpy array z >= 0 (support 2; include/sda_hip.h)."""
    import numpy as np
    z = np.asarray(z, np.float64)
    near = ((((-0.25 * z + 0.5) * z + 0.625) * z - 5.0 / 3.0) * z * z) + 1.0
    zf = np.where(z > 1.0, z, 1.0)                                    # (keeps 2 / (3 z) finite where the far branch is unused)
    far = ((((zf / 12.0 - 0.5) * zf + 0.625) * zf + 5.0 / 3.0) * zf - 5.0) * zf + 4.0 - 2.0 / (3.0 * zf)
    return np.where(z <= 1.0, near, np.where(z < 2.0, far, 0.0))


class EnklPlan:
    """What ``enkl_plan`` returns: the grid ``event`` (C, Hg, Wg), ``block`` (bh, bw), ``nblk``, ``k`` observed values, the CSR
    lists on the device (``offsets`` (nblk + 1,) int32, ``idx`` (nnz,) int32, ``rho`` (nnz,) fp32) and their host copies
    (``offsets_host`` ..., numpy).  Scratch of the weights launch is kept here per ensemble size."""

    def __init__(self, event, block, k, offsets, idx, rho, radius, device):
        self.event, self.block, self.k, self.radius = event, block, k, radius
        self.nblk = (event[1] // block[0]) * (event[2] // block[1])
        self.offsets_host, self.idx_host, self.rho_host = offsets, idx, rho
        self.device = torch.device(device)
        self.offsets = torch.from_numpy(offsets).to(self.device)
        self.idx = torch.from_numpy(idx).to(self.device) if idx.size else torch.zeros(1, dtype=torch.int32, device=self.device)
        self.rho = torch.from_numpy(rho).to(self.device) if rho.size else torch.zeros(1, dtype=torch.float32, device=self.device)
        self._scratch = {}

    @property
    def d(self) -> int:
        return self.event[0] * self.event[1] * self.event[2]

    def scratch(self, m: int):
        if m not in self._scratch:
            self._scratch = {m: (torch.empty(self.k, 2 * m, device=self.device, dtype=torch.float32),
                                 torch.empty(self.nblk * m * m, device=self.device, dtype=torch.float64))}
        return self._scratch[m]


def enkl_plan(event, positions, radius: float, block, *, device=None) -> EnklPlan:
    """The localisation plan of a run (include/sda_hip.h), built in float64 on the host and uploaded once.  ``event``: the state's
    shape (C, Hg, Wg), or (n,) for a ring (= (1, 1, n)); ``positions``: (k, 2) real-valued (row, col) of the observed values in
    their flattened order, (k,) on a ring; ``block``: (bh, bw), or an int on a ring; ``radius`` > 0 in grid points, the
    Gaspari-Cohn weight vanishes at twice that; ``float('inf')`` gives all-ones weights.  ``device`` defaults to the current HIP
    device."""
    import numpy as np
    event = tuple(int(e) for e in event)
    ring = len(event) == 1
    if ring:
        event = (1, 1, event[0])
        block = (1, int(block)) if not isinstance(block, (tuple, list)) else tuple(block)
        if len(block) == 1:
            block = (1, int(block[0]))
    if len(event) != 3 or min(event) < 1:
        raise _lib.SdaHipError(f'enkl_plan: event {event}, expected (C, Hg, Wg) or (n,)')
    block = tuple(int(v) for v in block) if isinstance(block, (tuple, list)) else None
    if block is None or len(block) != 2 or min(block) < 1 or event[1] % block[0] or event[2] % block[1]:
        raise _lib.SdaHipError(f'enkl_plan: block {block} does not divide the grid {event[1:]}')
    if not radius > 0:
        raise _lib.SdaHipError(f'enkl_plan: radius {radius}, expected > 0')
    pos = positions.detach().cpu().numpy() if isinstance(positions, Tensor) else np.asarray(positions)
    pos = pos.astype(np.float64)
    if ring and pos.ndim == 1:
        pos = np.stack([np.zeros_like(pos), pos], axis=1)
    if pos.ndim != 2 or pos.shape[1] != 2 or pos.shape[0] < 1 or not np.isfinite(pos).all():
        raise _lib.SdaHipError(f'enkl_plan: positions of shape {tuple(np.shape(positions))}, expected (k, 2)' +
                               (' or (k,) on a ring' if ring else ''))
    C, Hg, Wg = event
    bh, bw = block
    cr = np.arange(Hg // bh, dtype=np.float64) * bh + (bh - 1) / 2.0
    cc = np.arange(Wg // bw, dtype=np.float64) * bw + (bw - 1) / 2.0
    dr = np.abs(cr[:, None] - pos[None, :, 0]) % Hg
    dc = np.abs(cc[:, None] - pos[None, :, 1]) % Wg
    dr, dc = np.minimum(dr, Hg - dr), np.minimum(dc, Wg - dc)
    dist = np.sqrt(dr[:, None, :] ** 2 + dc[None, :, :] ** 2).reshape(-1, pos.shape[0])          # (nblk, k)
    rho = gaspari_cohn(dist / radius).astype(np.float32)
    keep = rho > 0
    offsets = np.zeros(dist.shape[0] + 1, np.int64)
    np.cumsum(keep.sum(axis=1), out=offsets[1:])
    if offsets[-1] > 0x7fffffff:
        raise _lib.SdaHipError(f'enkl_plan: {int(offsets[-1])} list entries (at most 2^31 - 1 are served)')
    idx = np.nonzero(keep)[1].astype(np.int32)
    if device is None:
        device = torch.device('cuda', torch.cuda.current_device())
    return EnklPlan(event, block, pos.shape[0], offsets.astype(np.int32), idx, np.ascontiguousarray(rho[keep]), float(radius), device)


def enkl_weights(plan: EnklPlan, Y: Tensor, D: Tensor, sigma: float, *, W: Optional[Tensor] = None, status: Optional[Tensor] = None):
    """Per block ``W`` (nblk, m, m) fp32 and ``status`` (nblk,) int32 (1: no Cholesky factor or a non-finite W[b]; W[b] is then zero)
    from ``enkw_prepare``'s Y, D (members, k): two launches (the pack and one workgroup per block), nothing read back."""
    _dev(Y, D)
    if Y.dim() != 2 or Y.shape != D.shape or not Y.is_contiguous() or not D.is_contiguous() or Y.shape[1] != plan.k:
        raise _lib.SdaHipError(f'enkl_weights: Y {tuple(Y.shape)} and D {tuple(D.shape)}, expected contiguous (members, {plan.k})')
    if Y.device != plan.device:
        raise _lib.SdaHipError(f'enkl_weights: Y on {Y.device}, the plan on {plan.device}')
    m, k = Y.shape
    if not 2 <= m <= ENKW_MAX_M:
        _lib.check(-2, 'sda_enkl_weights')
    if W is None:
        W = torch.empty(plan.nblk, m, m, device=Y.device, dtype=torch.float32)
    _dev(W)
    if tuple(W.shape) != (plan.nblk, m, m) or not W.is_contiguous():
        raise _lib.SdaHipError(f'enkl_weights: a contiguous ({plan.nblk}, {m}, {m}) fp32 device tensor expected for W')
    status = torch.zeros(plan.nblk, device=Y.device, dtype=torch.int32) if status is None else status
    if status.dtype != torch.int32 or tuple(status.shape) != (plan.nblk,) or not status.is_cuda or not status.is_contiguous():
        raise _lib.SdaHipError(f'enkl_weights: status ({plan.nblk},) int32 contiguous on the device expected')
    T, work = plan.scratch(m)
    lib = _lib.load()
    _lib.check(lib.sda_enkl_pack(Y.data_ptr(), D.data_ptr(), m, k, T.data_ptr(), _stream()), 'sda_enkl_pack')
    _lib.check(lib.sda_enkl_weights(T.data_ptr(), m, k, plan.offsets.data_ptr(), plan.idx.data_ptr(), plan.rho.data_ptr(), plan.nblk,
                                    float(sigma), work.data_ptr(), W.data_ptr(), status.data_ptr(), _stream()), 'sda_enkl_weights')
    return W, status


def enkl_transform(plan: EnklPlan, S: Tensor, lo: int, t: int, W: Tensor) -> Tensor:
    """The localised update, in place on the slabs ``S[lo] .. S[t]`` of the time-major ensemble S (time, members, C Hg Wg) with
    the per-block ``W`` (nblk, m, m), one launch.  Blocks with an empty list are not touched."""
    _enks_slabs(S, 'enkl_transform')
    if not 0 <= lo <= t < S.shape[0]:
        raise _lib.SdaHipError(f'enkl_transform: window {lo} .. {t} of {S.shape[0]} slabs')
    m, d = S.shape[1], S.shape[2]
    _dev(W)
    if d != plan.d or tuple(W.shape) != (plan.nblk, m, m) or not W.is_contiguous() or S.device != plan.device:
        raise _lib.SdaHipError(f'enkl_transform: slabs {tuple(S.shape)} and W {tuple(W.shape)} for a plan of {plan.nblk} blocks on '
                               f'{plan.event}, expected (time, m, {plan.d}) and contiguous ({plan.nblk}, m, m)')
    C, Hg, Wg = plan.event
    _lib.check(_lib.load().sda_enkl_transform(S[lo].data_ptr(), S.stride(0), S.stride(1), t - lo + 1, m, C, Hg, Wg, plan.block[0],
                                              plan.block[1], plan.offsets.data_ptr(), W.data_ptr(), _stream()), 'sda_enkl_transform')
    return S


def enkl_check(status: Tensor) -> None:
    """Raise if a block of any analysis had no Cholesky factor or a non-finite transform; status (N, nblk)."""
    bad = status.nonzero().tolist()
    if bad:
        raise _lib.SdaHipError(f'localised ensemble Kalman smoother: {len(bad)} block solve(s) failed, the first at (observation, '
                               f'block) {tuple(bad[0])}')


# ---------------------------------------------------------------- Kolmogorov flow (csrc/kflow.hip)
_KFLOW_CONST = {}
_KFLOW_SOLVE = {}


def kflow_serves(n: int) -> bool:
    """The sizes the kernels take: n % 16 == 0, 16 <= n <= 512."""
    return bool(_lib.load().sda_kflow_serves(int(n)))


def kflow_device_key(device):
    """(type, index) of `device` with an unnamed HIP index resolved to the current device: what the per-device caches are keyed
    on, so a cached table never outlives a change of the current device."""
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        return device.type, torch.cuda.current_device()
    return device.type, device.index


def _kflow_solve_tables(n: int):
    """Host float64: 1 / (lam_a + lam_b) with 0 for the mean mode (n, n), and the forcing profile sin(4 (j + 1/2) h) (n,)."""
    k = torch.arange(n, dtype=torch.float64)
    h = 2 * math.pi / n
    lam = (2 * (2 * math.pi * k / n).cos() - 2) / (h * h)
    s = lam[:, None] + lam[None, :]
    s[0, 0] = 1.0
    inv = 1 / s
    inv[0, 0] = 0.0
    forcing = (4 * (k + 0.5) * h).sin()
    return inv, forcing


def kflow_tables(n: int):
    """Host float64 tables of size n: the Hartley matrix Hm (n, n), 1 / (lam_a + lam_b) with 0 for the mean mode (n, n), and the
    forcing profile sin(4 (j + 1/2) h) (n,)."""
    k = torch.arange(n, dtype=torch.int64)
    ang = 2 * math.pi * ((k[:, None] * k[None, :]) % n).double() / n
    hm = (ang.cos() + ang.sin()) / math.sqrt(n)
    inv, forcing = _kflow_solve_tables(n)
    return hm, inv, forcing


def kflow_solve_tables(n: int, device, dtype):
    """(inv, forcing) of `kflow_tables` on `device` in `dtype`, built once per (n, device, dtype): what the torch-ops route reads
    every sub-step.  Hm is not built for it."""
    device = torch.device(device)
    key = (n, *kflow_device_key(device), dtype)
    c = _KFLOW_SOLVE.get(key)
    if c is None:
        c = _KFLOW_SOLVE[key] = tuple(t.to(device=device, dtype=dtype) for t in _kflow_solve_tables(n))
    return c


def kflow_constants(n: int, device) -> Tensor:
    """[Hm | inv | forcing] of size n on `device`, built once in float64 on the host and rounded."""
    device = torch.device(device)
    key = (n, *kflow_device_key(device))
    c = _KFLOW_CONST.get(key)
    if c is None:
        hm, inv, forcing = kflow_tables(n)
        c = _KFLOW_CONST[key] = torch.cat([hm.flatten(), inv.flatten(), forcing]).float().to(device)
    return c


def kflow_model(n: int, steps: int, delta: float, nu: float, device) -> '_lib.KflowModel':
    """`sda_kflow_model`: delta = dt / steps and nu rounded to fp32 once."""
    if not kflow_serves(n):
        raise _lib.SdaHipError(f'kflow: size {n} is not served by the kernels (n % 16 == 0, 16 <= n <= 512)')
    c = kflow_constants(n, device)
    m = _lib.KflowModel()
    m.n, m.steps, m.delta, m.nu = int(n), int(steps), float(delta), float(nu)
    m.hm, m.inv, m.forcing = c.data_ptr(), c.data_ptr() + 4 * n * n, c.data_ptr() + 8 * n * n
    m._keep = c
    return m


def _kflow_fields(x: Tensor, n: int, planes: int, what: str):
    """x (..., planes, n, n) -> (nb, planes, n, n) whose fields are dense and 16-byte aligned (the batch stride is free)."""
    _dev(x)
    if x.dim() < 3 or tuple(x.shape[-3:]) != (planes, n, n) or x.numel() == 0:
        raise _lib.SdaHipError(f'{what}: fields of shape {tuple(x.shape)}, expected (..., {planes}, {n}, {n})')
    f = x.reshape(-1, planes, n, n)
    sb = f.stride(0) if f.shape[0] > 1 else planes * n * n
    dense = f.stride()[2:] == (n, 1) and (planes == 1 or f.stride(1) == n * n)
    if not dense or sb < planes * n * n or sb % 4 or f.data_ptr() % 16:
        f = f.contiguous()
        sb = planes * n * n
    if f.shape[0] > 65535:
        raise _lib.SdaHipError(f'{what}: {f.shape[0]} fields in one call (at most 65535)')
    return f, sb


def kflow_explicit(model, x: Tensor) -> Tensor:
    """x (..., 2, n, n) -> (u*, v*) = x + delta (-adv + nu lap + f), one launch."""
    f, sb = _kflow_fields(x, model.n, 2, 'kflow_explicit')
    out = torch.empty(f.shape, device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().sda_kflow_explicit(ctypes.byref(model), f.data_ptr(), sb, f.shape[0], out.data_ptr(), _stream()),
               'sda_kflow_explicit')
    return out.reshape(x.shape)


def kflow_hartley(x: Tensor, scale: Optional[Tensor] = None) -> Tensor:
    """x (..., n, n) -> (Hm x Hm) o scale on the fp32 matrix cores (two launches); scale (n, n) or None.  Hm is its own inverse."""
    n = x.shape[-1]
    if not kflow_serves(n):
        raise _lib.SdaHipError(f'kflow_hartley: size {n} is not served (n % 16 == 0, 16 <= n <= 512)')
    f, sb = _kflow_fields(x.unsqueeze(-3), n, 1, 'kflow_hartley')
    if scale is not None:
        _dev(scale)
        if tuple(scale.shape) != (n, n) or not scale.is_contiguous():
            raise _lib.SdaHipError(f'kflow_hartley: scale {tuple(scale.shape)}, expected a contiguous ({n}, {n})')
    hm = kflow_constants(n, x.device)
    tmp = torch.empty(f.shape, device=x.device, dtype=torch.float32)
    out = torch.empty(f.shape, device=x.device, dtype=torch.float32)
    lib = _lib.load()
    _lib.check(lib.sda_kflow_hartley(hm.data_ptr(), n, f.data_ptr(), sb, f.shape[0], 0, None, tmp.data_ptr(), _stream()), 'sda_kflow_hartley')
    _lib.check(lib.sda_kflow_hartley(hm.data_ptr(), n, tmp.data_ptr(), n * n, f.shape[0], 1, _ptr(scale), out.data_ptr(), _stream()),
               'sda_kflow_hartley')
    return out.reshape(x.shape)


def kflow_project(model, x: Tensor) -> Tensor:
    """x (..., 2, n, n) -> x - grad(lap^-1 div x): the divergence-free part (four launches)."""
    n = model.n
    f, sb = _kflow_fields(x, n, 2, 'kflow_project')
    nb = f.shape[0]
    out = torch.empty(f.shape, device=x.device, dtype=torch.float32)
    work = torch.empty(2 * nb * n * n, device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().sda_kflow_project(ctypes.byref(model), f.data_ptr(), sb, nb, out.data_ptr(), 2 * n * n, work.data_ptr(),
                                             _stream()), 'sda_kflow_project')
    return out.reshape(x.shape)


def kflow_advance(model, x: Tensor, transitions: int, every: bool = False) -> Tensor:
    """x (nb..., 2, n, n) -> the state after `transitions` transitions (every=False), or (transitions, nb..., 2, n, n) with every
    kept frame written straight into its slab.  All transitions x steps sub-steps are queued; nothing is read back."""
    n = model.n
    f, sb = _kflow_fields(x, n, 2, 'kflow_advance')
    nb = f.shape[0]
    if transitions < 1:
        raise _lib.SdaHipError(f'kflow_advance: {transitions} transitions')
    lib = _lib.load()
    out = torch.empty((transitions, *x.shape) if every else tuple(x.shape), device=x.device, dtype=torch.float32)
    work = torch.empty(lib.sda_kflow_work_floats(n, nb), device=x.device, dtype=torch.float32)
    _lib.check(lib.sda_kflow_advance(ctypes.byref(model), f.data_ptr(), sb, nb, transitions, int(every), out.data_ptr(), nb * 2 * n * n,
                                     work.data_ptr(), _stream()), 'sda_kflow_advance')
    return out


def _kflow_pair(model, x: Tensor, g: Tensor, what: str):
    if g.shape != x.shape or g.device != x.device:
        raise _lib.SdaHipError(f'{what}: cotangent {tuple(g.shape)} on {g.device} for states {tuple(x.shape)} on {x.device}')
    if x.dtype != torch.float32 or g.dtype != torch.float32:
        raise _lib.SdaHipError(f'{what}: float32 states and cotangents, got {x.dtype} and {g.dtype}')
    return _kflow_fields(x, model.n, 2, what), _kflow_fields(g, model.n, 2, what)


def kflow_explicit_vjp(model, x: Tensor, g: Tensor) -> Tensor:
    """(d kflow_explicit / dx at x)^T g, both (..., 2, n, n): one launch, gather form (bitwise reproducible)."""
    (f, sb), (gf, gsb) = _kflow_pair(model, x, g, 'kflow_explicit_vjp')
    out = torch.empty(f.shape, device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().sda_kfvjp_explicit(ctypes.byref(model), f.data_ptr(), sb, gf.data_ptr(), gsb, f.shape[0], out.data_ptr(),
                                              _stream()), 'sda_kfvjp_explicit')
    return out.reshape(x.shape)


def kflow_transition_vjp(model, x0: Tensor, g: Tensor) -> Tensor:
    """(d transition / dx0 at x0)^T g, both (..., 2, n, n): the sub-step states are recomputed from x0 into one slab, then the
    sub-steps run backwards (five launches each, as forward).  All queued; nothing is read back."""
    (f, sb), (gf, gsb) = _kflow_pair(model, x0, g, 'kflow_transition_vjp')
    nb = f.shape[0]
    lib = _lib.load()
    out = torch.empty(f.shape, device=x0.device, dtype=torch.float32)
    work = torch.empty(lib.sda_kfvjp_work_floats(model.n, nb, model.steps), device=x0.device, dtype=torch.float32)
    _lib.check(lib.sda_kfvjp_transition(ctypes.byref(model), f.data_ptr(), sb, gf.data_ptr(), gsb, nb, out.data_ptr(), work.data_ptr(),
                                        _stream()), 'sda_kfvjp_transition')
    return out.reshape(x0.shape)


# ---------------------------------------------------------------- linear-Gaussian state space (csrc/lgss.hip)
def _lgss_f64(a, shape, what: str):
    t = torch.as_tensor(a, dtype=torch.float64, device='cpu') if not torch.is_tensor(a) else a.detach().to('cpu', torch.float64)
    if tuple(t.shape) != tuple(shape) or not torch.isfinite(t).all():
        raise _lib.SdaHipError(f'lgss: {what} of shape {tuple(t.shape)}, expected finite {tuple(shape)}')
    return t


def _lgss_fill(field, t):
    if t.dim() == 1:
        for i, v in enumerate(t.tolist()):
            field[i] = v
    else:
        for i, row in enumerate(t.tolist()):
            for j, v in enumerate(row):
                field[i][j] = v


def lgss_model(A, b, Q) -> '_lib.LgssModel':
    """`sda_lgss_model` of x' = A x + b + w, w ~ N(0, Q): fp32 A, b and the lower Cholesky factor of Q (formed in float64, rounded once)."""
    b = torch.as_tensor(b)
    d = b.numel()
    if not 1 <= d <= _lib.LGSS_MAXD:
        raise _lib.SdaHipError(f'lgss_model: d = {d}, the kernels serve 1 <= d <= {_lib.LGSS_MAXD}')
    A, b, Q = _lgss_f64(A, (d, d), 'A'), _lgss_f64(b, (d,), 'b'), _lgss_f64(Q, (d, d), 'Q')
    Lq, info = torch.linalg.cholesky_ex(Q)
    if int(info) != 0:
        raise _lib.SdaHipError('lgss_model: Q is not positive definite')
    m = _lib.LgssModel()
    m.d = d
    _lgss_fill(m.A, A)
    _lgss_fill(m.b, b)
    _lgss_fill(m.Lq, Lq)
    return m


def lgss_model64(A, b, Q, m0, P0, H, c, sigma: float) -> '_lib.LgssModel64':
    """`sda_lgss_model64`: the chain, the law N(m0, P0) of the state at time index 0 and the observation y = H x + c + N(0, sigma^2 I)."""
    b = torch.as_tensor(b)
    c = torch.as_tensor(c)
    d, k = b.numel(), c.numel()
    if not (1 <= d <= _lib.LGSS_MAXD and 1 <= k <= _lib.LGSS_MAXD) or not float(sigma) > 0:
        raise _lib.SdaHipError(f'lgss_model64: d = {d}, k = {k}, sigma = {sigma}: the kernels serve 1 <= d, k <= {_lib.LGSS_MAXD}, sigma > 0')
    m = _lib.LgssModel64()
    m.d, m.k, m.sigma = d, k, float(sigma)
    for name, val, shape in (('A', A, (d, d)), ('b', b, (d,)), ('Q', Q, (d, d)), ('m0', m0, (d,)), ('P0', P0, (d, d)), ('H', H, (k, d)),
                             ('c', c, (k,))):
        _lgss_fill(getattr(m, name), _lgss_f64(val, shape, name))
    return m


def lgss_advance(model, x: Tensor, out: Tensor, transitions: int, *, every: bool = False, out_st: int = 0, out_sp: Optional[int] = None,
                 seed: int = 0, row0: int = 0, draw0: int = 0) -> Tensor:
    """`transitions` transitions of x (m, d) in one launch; `out` and its strides as in ``chain_advance``."""
    _dev(x, out)
    m, d = x.shape
    if x.dim() != 2 or x.stride(1) != 1 or d != model.d:
        raise _lib.SdaHipError(f'lgss_advance: states {tuple(x.shape)} (strides {x.stride()}) for a {model.d}-component chain')
    out_sp = d if out_sp is None else out_sp
    last = (transitions - 1) * out_st if every else 0
    if out_sp < d or (every and out_st < 0) or last + (m - 1) * out_sp + d > out.numel() or not out.is_contiguous():
        raise _lib.SdaHipError('lgss_advance: the output strides leave the output tensor')
    _lib.check(_lib.load().sda_lgss_advance(ctypes.byref(model), x.data_ptr(), x.stride(0) if m > 1 else d, m, transitions, int(every),
                                            out.data_ptr(), out_st, out_sp, seed & 0xffffffffffffffff, row0, draw0, _stream()),
               'sda_lgss_advance')
    return out


def lgss_tables(model64, step: int, n_obs: int, device=None, lib=None) -> Tensor:
    """The Kalman / backward-sampler tables of `n_obs` observations `step` apart (host call, float64), uploaded to `device` if given.
    ``lib``: another library exporting ``sda_lgss_tables`` (the host replay of the tests)."""
    lib = _lib.load() if lib is None else lib
    T = (n_obs - 1) * step
    n = lib.sda_lgss_table_doubles(model64.d, model64.k, T) if n_obs >= 1 and step >= 1 else -1
    if n < 0:
        raise _lib.SdaHipError(f'lgss_tables: {n_obs} observations, step {step}')
    table = torch.empty(n, dtype=torch.float64)
    _lib.check(lib.sda_lgss_tables(ctypes.byref(model64), step, n_obs, table.data_ptr()), 'sda_lgss_tables (a covariance is not positive definite?)')
    return table if device is None else table.to(device)


def _lgss_table_check(model64, table: Tensor, T: int, what: str):
    want = _lib.load().sda_lgss_table_doubles(model64.d, model64.k, T)
    if not table.is_cuda or table.dtype != torch.float64 or not table.is_contiguous() or table.numel() != want:
        raise _lib.SdaHipError(f'{what}: the table must be {want} contiguous float64 values on the device')


def lgss_filter(model64, table: Tensor, y: Tensor, step: int):
    """y (B, N, k) fp32 -> (mean (B, T + 1, d), logz (B,)), float64: the filtered means and log p(y)."""
    _dev(y)
    if y.dim() != 3 or y.shape[2] != model64.k or y.shape[0] < 1 or y.shape[1] < 1 or step < 1:
        raise _lib.SdaHipError(f'lgss_filter: observations {tuple(y.shape)} for k = {model64.k}, step {step}')
    y = y.contiguous()
    B, N = y.shape[:2]
    T = (N - 1) * step
    _lgss_table_check(model64, table, T, 'lgss_filter')
    mean = torch.empty(B, T + 1, model64.d, device=y.device, dtype=torch.float64)
    logz = torch.empty(B, device=y.device, dtype=torch.float64)
    _lib.check(_lib.load().sda_lgss_filter(ctypes.byref(model64), table.data_ptr(), step, N, y.data_ptr(), B, mean.data_ptr(),
                                           logz.data_ptr(), _stream()), 'sda_lgss_filter')
    return mean, logz


def lgss_sample(model64, table: Tensor, mean: Tensor, samples: int, seed: int, row0: int = 0, draw0: int = 0) -> Tensor:
    """mean (B, T + 1, d) float64 -> (B, samples, T + 1, d) fp32 exact posterior trajectories; sample (b, r) at time i uses row
    row0 + b * samples + r of the keyed normals at draw0 + i."""
    if mean.dim() != 3 or not mean.is_cuda or mean.dtype != torch.float64 or not mean.is_contiguous() or mean.shape[2] != model64.d \
            or samples < 1:
        raise _lib.SdaHipError(f'lgss_sample: means {tuple(mean.shape)} ({mean.dtype}) for d = {model64.d}, {samples} samples')
    B, T = mean.shape[0], mean.shape[1] - 1
    _lgss_table_check(model64, table, T, 'lgss_sample')
    out = torch.empty(B, samples, T + 1, model64.d, device=mean.device, dtype=torch.float32)
    _lib.check(_lib.load().sda_lgss_sample(ctypes.byref(model64), table.data_ptr(), mean.data_ptr(), T, B, samples,
                                           seed & 0xffffffffffffffff, row0, draw0, out.data_ptr(), _stream()), 'sda_lgss_sample')
    return out


def lgss_score_prec(A, b, Q, m0, P0, T: int) -> Tensor:
    """The `prec` operand of the exact score (host, float64): {P0^-1, Q^-1, A^T Q^-1, A^T Q^-1 A, mean[T + 1][d]} of the joint law of
    (x_0 .. x_T), x_0 ~ N(m0, P0)."""
    b = torch.as_tensor(b)
    d = b.numel()
    A, b, Q = _lgss_f64(A, (d, d), 'A'), _lgss_f64(b, (d,), 'b'), _lgss_f64(Q, (d, d), 'Q')
    m0, P0 = _lgss_f64(m0, (d,), 'm0'), _lgss_f64(P0, (d, d), 'P0')
    Qi, Si = torch.linalg.inv(Q), torch.linalg.inv(P0)
    Qi, Si = 0.5 * (Qi + Qi.T), 0.5 * (Si + Si.T)
    AtQi = A.T @ Qi
    AtQiA = AtQi @ A
    mean = [m0]
    for _ in range(T):
        mean.append(A @ mean[-1] + b)
    return torch.cat([Si.reshape(-1), Qi.reshape(-1), AtQi.reshape(-1), (0.5 * (AtQiA + AtQiA.T)).reshape(-1), torch.stack(mean).reshape(-1)])


def _lgss_score_check(d: int, T: int, prec: Tensor, coef: Tensor, work: Tensor, what: str):
    lib = _lib.load()
    if not 1 <= d <= _lib.LGSS_MAXD or T < 0:
        raise _lib.SdaHipError(f'{what}: d = {d}, T = {T}')
    for t, n, dt, name in ((prec, lib.sda_lgss_score_doubles(d, T, 0), torch.float64, 'prec'), (coef, 2, torch.float32, 'coef'),
                           (work, lib.sda_lgss_score_doubles(d, T, 1), torch.float64, 'work')):
        if not t.is_cuda or t.dtype != dt or not t.is_contiguous() or t.numel() != n:
            raise _lib.SdaHipError(f'{what}: {name} must be {n} contiguous {dt} values on the device')


def lgss_score_factor(d: int, T: int, prec: Tensor, coef: Tensor, work: Optional[Tensor] = None) -> Tensor:
    """Block Cholesky of mu^2 I + sigma^2 Lambda, {mu, sigma} = coef read on the device (a captured step replays)."""
    if work is None:
        work = torch.empty(_lib.load().sda_lgss_score_doubles(d, T, 1), device=prec.device, dtype=torch.float64)
    _lgss_score_check(d, T, prec, coef, work, 'lgss_score_factor')
    _lib.check(_lib.load().sda_lgss_score_factor(d, T, prec.data_ptr(), coef.data_ptr(), work.data_ptr(), _stream()),
               'sda_lgss_score_factor')
    return work


def lgss_score(d: int, T: int, prec: Tensor, coef: Tensor, work: Tensor, x: Tensor, zero_mean: bool = False) -> Tensor:
    """x (n, T + 1, d) fp32 -> eps likewise.  zero_mean: the same map around m = 0, which is also its own transpose (the VJP)."""
    _dev(x)
    _lgss_score_check(d, T, prec, coef, work, 'lgss_score')
    if x.dim() != 3 or tuple(x.shape[1:]) != (T + 1, d) or x.shape[0] < 1:
        raise _lib.SdaHipError(f'lgss_score: trajectories {tuple(x.shape)}, expected (n, {T + 1}, {d})')
    x = x.contiguous()
    n = x.shape[0]
    ywork = torch.empty(n * (T + 1) * d, device=x.device, dtype=torch.float64)
    out = torch.empty_like(x)
    _lib.check(_lib.load().sda_lgss_score(d, T, prec.data_ptr(), coef.data_ptr(), work.data_ptr(), x.data_ptr(), n, int(zero_mean),
                                          ywork.data_ptr(), out.data_ptr(), _stream()), 'sda_lgss_score')
    return out
