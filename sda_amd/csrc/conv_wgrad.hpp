// Planner and index helpers of the convolution weight gradient, shared by the general kernel (conv_wgrad.hip), the tiled 3 x 3
// kernel (conv_wgrad3.hip) and their host replays (libsda_emu.so): the geometry, the column / position decoders, the loader that
// rebuilds the layer's input V as its forward launch saw it, and the slab-ordered reduction of one element.
#pragma once
#include "sda_common.hpp"

#define WG_THREADS 256
#define WG_KP 32                 // positions per stage
#define WG_BN 128                // columns per workgroup (4 waves x 32)
#define WG_MAX_SLABS 64
#define WG_TARGET_BLOCKS 2048    // enough workgroups to fill 256 CUs several times over

struct WgradGeom {
    int cin;             // cx + cctx
    int hv, wv;          // virtual input size (after up-sampling)
    int pad_h, pad_w;
    int ntaps, ncol;     // ncol = cin*ntaps + 1
    int mt, bm, n_ct, n_colt;
    int64_t P;           // n*ho*wo
    int hw_o;            // ho*wo
    int slabs;
    int64_t per;         // positions per slab (multiple of WG_KP)
    int grid;
};

static inline int wgrad_plan(const sda_wgrad_desc* wd, WgradGeom* g) {
    if (!wd || !wd->g || !wd->dw || !wd->work) return SDA_E_BADARG;
    const sda_conv_desc* d = &wd->conv;
    if (!d->x) return SDA_E_BADARG;
    if (d->n <= 0 || d->cx <= 0 || d->cout <= 0 || d->hs <= 0 || d->ws <= 0 || d->ho <= 0 || d->wo <= 0) return SDA_E_BADARG;
    if (d->kh <= 0 || d->kw <= 0) return SDA_E_UNSUPPORTED;
    if (!d->explicit_pad && (!(d->kh & 1) || !(d->kw & 1))) return SDA_E_UNSUPPORTED;
    if (d->explicit_pad && (d->pad_h < 0 || d->pad_w < 0 || d->pad_h >= d->kh || d->pad_w >= d->kw)) return SDA_E_BADARG;
    if (d->stride_h < 1 || d->stride_w < 1 || d->up_h < 1 || d->up_w < 1) return SDA_E_UNSUPPORTED;
    if ((d->zins_h > 1 || d->zins_w > 1) || (d->pool_h > 1 || d->pool_w > 1)) return SDA_E_UNSUPPORTED;
    if (d->cctx > 0 && !d->ctx) return SDA_E_BADARG;
    if ((d->ln_mean == nullptr) != (d->ln_rstd == nullptr)) return SDA_E_BADARG;
    if (d->n_inner < 1) return SDA_E_BADARG;
    if (wd->slabs < 0 || wd->slabs > WG_MAX_SLABS) return SDA_E_BADARG;
    g->cin = d->cx + (d->cctx > 0 ? d->cctx : 0);
    g->hv = d->hs * d->up_h;
    g->wv = d->ws * d->up_w;
    g->pad_h = d->explicit_pad ? d->pad_h : d->kh / 2;
    g->pad_w = d->explicit_pad ? d->pad_w : d->kw / 2;
    g->ntaps = d->kh * d->kw;
    const int64_t ncol = (int64_t)g->cin * g->ntaps + 1;
    if (ncol > (1 << 24)) return SDA_E_UNSUPPORTED;
    g->ncol = (int)ncol;
    g->mt = d->cout > 96 ? 4 : (d->cout + 31) / 32;
    g->bm = 32 * g->mt;
    g->n_ct = (d->cout + g->bm - 1) / g->bm;
    g->n_colt = (g->ncol + WG_BN - 1) / WG_BN;
    g->hw_o = d->ho * d->wo;
    g->P = (int64_t)d->n * g->hw_o;
    const int64_t stages = (g->P + WG_KP - 1) / WG_KP;
    const int64_t tiles = (int64_t)g->n_ct * g->n_colt;
    int64_t s = wd->slabs;
    if (s == 0) {                                            // the planner's choice: a function of the shape only
        s = (WG_TARGET_BLOCKS + tiles - 1) / tiles;
        if (s > WG_MAX_SLABS) s = WG_MAX_SLABS;
    }
    if (s > stages) s = stages;
    if (s < 1) s = 1;
    g->per = (stages + s - 1) / s * WG_KP;
    g->slabs = (int)((g->P + g->per - 1) / g->per);          // (no empty slab)
    if (tiles * g->slabs > 0x7fffffffL) return SDA_E_UNSUPPORTED;
    g->grid = (int)(tiles * g->slabs);
    return SDA_OK;
}

// ---------------------------------------------------------------- index helpers (host + device)

__host__ __device__ inline int wgrad_wrap(int v, int m) {
    v %= m;
    return v < 0 ? v + m : v;
}

// D-fragment row of accumulator register r for v_mfma_f32_32x32x2_f32 (col = lane & 31)
__host__ __device__ inline int wgrad_mfma_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// workgroup b -> (slab, cout tile, column tile)
__host__ __device__ inline void wgrad_decode_block(const WgradGeom& g, int b, int& slab, int& ct, int& colt) {
    colt = b % g.n_colt;
    int r = b / g.n_colt;
    ct = r % g.n_ct;
    slab = r / g.n_ct;
}

// column j of the GEMM -> (input channel, tap offsets); ci = -2: the ones column (bias), ci = -1: beyond the matrix
struct WgradCol {
    int ci, dy, dx;
};
__host__ __device__ inline WgradCol wgrad_decode_col(const sda_conv_desc& d, const WgradGeom& g, int j) {
    WgradCol c;
    c.dy = 0; c.dx = 0;
    if (j >= g.ncol) { c.ci = -1; return c; }
    if (j == g.ncol - 1) { c.ci = -2; return c; }
    c.ci = j / g.ntaps;
    int tap = j - c.ci * g.ntaps;
    int ky = tap / d.kw;
    c.dy = ky - g.pad_h;
    c.dx = tap - ky * d.kw - g.pad_w;
    return c;
}

// output position p (< P) -> image, row, column
struct WgradPos {
    int n, oy, ox;
};
__host__ __device__ inline WgradPos wgrad_decode_pos(const sda_conv_desc& d, const WgradGeom& g, int64_t p) {
    WgradPos r;
    r.n = (int)(p / g.hw_o);
    int pix = (int)(p - (int64_t)r.n * g.hw_o);
    r.oy = pix / d.wo;
    r.ox = pix - r.oy * d.wo;
    return r;
}

// cotangent g[n][co][oy][ox]
__host__ __device__ inline float wgrad_load_g(const sda_wgrad_desc& wd, const WgradGeom& g, const WgradPos& ps, int co) {
    if (co >= wd.conv.cout) return 0.f;
    return wd.g[((int64_t)ps.n * wd.conv.cout + co) * g.hw_o + (int64_t)ps.oy * wd.conv.wo + ps.ox];
}

// the loader's value of channel ci (>= 0) of image n at the SOURCE pixel (sy, sx), both in range: source view or context plane,
// + modulation -> LayerNorm -> activation
__host__ __device__ inline float wgrad_load_src(const sda_conv_desc& d, int n, int ci, int sy, int sx) {
    float v;
    if (ci < d.cx) {
        const int m = n + d.x_n_off;
        const int64_t nbase = (int64_t)(m / d.n_inner) * d.x_sn_outer + (int64_t)(m % d.n_inner) * d.x_sn_inner;
        v = d.x[nbase + (int64_t)sy * d.x_sy + (int64_t)sx * d.x_sx + (int64_t)ci * d.x_sc];
        if (d.mod) v += d.mod[(int64_t)n * d.mod_sn + ci];
        if (d.ln_mean) {
            const int64_t st = (int64_t)n * d.hs * d.ws + (int64_t)sy * d.ws + sx;
            v = (v - d.ln_mean[st]) * d.ln_rstd[st];
        }
    } else {
        v = d.ctx[(int64_t)n * d.ctx_sn + (int64_t)sy * d.ws + sx + (int64_t)(ci - d.cx) * d.hs * d.ws];
    }
    if (d.act_in) v = sda_act(d.act_in, v);
    return v;
}

// V(n, ci, oy*stride + dy, ox*stride + dx): the forward loader's value (sda_conv_desc semantics, as conv_igemm's loader)
__host__ __device__ inline float wgrad_load_v(const sda_conv_desc& d, const WgradGeom& g, const WgradPos& ps, const WgradCol& c) {
    if (c.ci < 0) return c.ci == -2 ? 1.f : 0.f;
    int vy = ps.oy * d.stride_h + c.dy;
    int vx = ps.ox * d.stride_w + c.dx;
    if (d.circular) {
        vy = wgrad_wrap(vy, g.hv);
        vx = wgrad_wrap(vx, g.wv);
    } else if (vy < 0 || vy >= g.hv || vx < 0 || vx >= g.wv) {
        return 0.f;
    }
    return wgrad_load_src(d, ps.n, c.ci, vy / d.up_h, vx / d.up_w);
}

// reduction of element e = co*ncol + j over the slabs, in slab order
__host__ __device__ inline void wgrad_reduce_one(const sda_wgrad_desc& wd, const WgradGeom& g, int64_t e) {
    const int64_t stride = (int64_t)wd.conv.cout * g.ncol;
    float s = 0.f;
    for (int k = 0; k < g.slabs; ++k) s += wd.work[(int64_t)k * stride + e];
    const int co = (int)(e / g.ncol);
    const int j = (int)(e - (int64_t)co * g.ncol);
    if (j < g.ncol - 1) {
        float* o = wd.dw + (int64_t)co * (g.ncol - 1) + j;
        *o = wd.accumulate ? *o + s : s;
    } else if (wd.db) {
        float* o = wd.db + co;
        *o = wd.accumulate ? *o + s : s;
    }
}

#ifndef SDA_HOST_EMU
// the slab-order reduction of work[slab][co][col] into dw / db (conv_wgrad.hip; g.slabs, g.ncol and the descriptor are all it reads)
int wgrad_launch_reduce(const sda_wgrad_desc* d, const WgradGeom& g, hipStream_t stream);
#endif
