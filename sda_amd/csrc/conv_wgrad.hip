// Weight gradient of one convolution layer on the fp32 matrix cores (the parameter half of the backward pass).
//
//   dW[co][ci][ky][kx] (+)= sum_{n,oy,ox} g[n][co][oy][ox] * V(n, ci, oy*stride_h + ky - pad_h, ox*stride_w + kx - pad_w)
//   db[co]             (+)= sum_{n,oy,ox} g[n][co][oy][ox]
//
// An implicit GEMM with M = cout, N = cin*kh*kw + 1 (the last column is the constant 1: db falls out of the same multiply)
// and the contraction over P = n*ho*wo output positions.  V is the layer's input exactly as its forward loader saw it
// (sda_conv_desc: strided / sliding-window source view, context channels, modulation + LayerNorm, activation, nearest
// up-sample, circular or zero padding), rebuilt on the fly -- nothing is materialised.
//
// Design:
//   * the position axis is cut into `slabs` contiguous ranges; workgroup (slab, cout tile, column tile) owns a 32*MT x 128 tile
//     of the result over its slab and writes it, unreduced, to work[slab][co][col];
//   * per stage of 32 positions the workgroup stages g[32 pos][BM couts] and V[32 pos][128 cols] into LDS (rows padded by one
//     float: the staging writes run down a column), then each of the 4 waves issues v_mfma_f32_32x32x2_f32 over its 32 columns:
//     A = g[co = lane&31][k = lane>>5], B = V[k = lane>>5][col = lane&31], D row = mfma32_row(r, lane), col = lane&31;
//   * a second kernel sums the slabs in slab order (no atomics anywhere: bitwise reproducible) and writes or adds dW, db.
//
// Index arithmetic is in __host__ __device__ helpers; the emulator at the bottom (libsda_emu.so, tests only) replays the
// planner, the staging maps, the MFMA lane maps and the reduction order on the CPU.
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

static int wgrad_plan(const sda_wgrad_desc* wd, WgradGeom* g) {
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
    const int sy = vy / d.up_h, sx = vx / d.up_w;
    float v;
    if (c.ci < d.cx) {
        const int m = ps.n + d.x_n_off;
        const int64_t nbase = (int64_t)(m / d.n_inner) * d.x_sn_outer + (int64_t)(m % d.n_inner) * d.x_sn_inner;
        v = d.x[nbase + (int64_t)sy * d.x_sy + (int64_t)sx * d.x_sx + (int64_t)c.ci * d.x_sc];
        if (d.mod) v += d.mod[(int64_t)ps.n * d.mod_sn + c.ci];
        if (d.ln_mean) {
            const int64_t st = (int64_t)ps.n * d.hs * d.ws + (int64_t)sy * d.ws + sx;
            v = (v - d.ln_mean[st]) * d.ln_rstd[st];
        }
    } else {
        v = d.ctx[(int64_t)ps.n * d.ctx_sn + (int64_t)sy * d.ws + sx + (int64_t)(c.ci - d.cx) * d.hs * d.ws];
    }
    if (d.act_in) v = sda_act(d.act_in, v);
    return v;
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

#define WG_ROW_G(bm) ((bm) + 1)  // LDS row pitch (floats) of the staged cotangent
#define WG_ROW_V (WG_BN + 1)     // ... and of the staged input

// ---------------------------------------------------------------- the kernels
#ifndef SDA_HOST_EMU

typedef float wg_f32x16 __attribute__((ext_vector_type(16)));

template <int MT>
__global__ __launch_bounds__(WG_THREADS) void conv_wgrad_kernel(const sda_wgrad_desc wd, const WgradGeom g) {
    constexpr int BM = 32 * MT;
    constexpr int RG = WG_ROW_G(BM);
    constexpr int NCOL_T = WG_BN / (WG_THREADS / WG_KP);          // columns staged per thread (16)
    constexpr int NCO_T = BM / (WG_THREADS / WG_KP);              // couts staged per thread (4 MT)
    __shared__ float s_g[WG_KP * RG];
    __shared__ float s_v[WG_KP * WG_ROW_V];
    const sda_conv_desc& d = wd.conv;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int l31 = lane & 31;
    const int khalf = lane >> 5;
    int slab, ct, colt;
    wgrad_decode_block(g, blockIdx.x, slab, ct, colt);
    const int co0 = ct * BM;
    const int col0 = colt * WG_BN;

    // staging roles: position lane pi, column / cout group cg
    const int pi = tid & (WG_KP - 1);
    const int cg = tid / WG_KP;
    WgradCol cols[NCOL_T];
#pragma unroll
    for (int i = 0; i < NCOL_T; ++i) cols[i] = wgrad_decode_col(d, g, col0 + cg + 8 * i);

    wg_f32x16 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;

    const int64_t p_begin = (int64_t)slab * g.per;
    const int64_t p_end = p_begin + g.per < g.P ? p_begin + g.per : g.P;
    for (int64_t p0 = p_begin; p0 < p_end; p0 += WG_KP) {
        const int64_t p = p0 + pi;
        const bool valid = p < p_end;
        WgradPos ps;
        ps.n = 0; ps.oy = 0; ps.ox = 0;
        if (valid) ps = wgrad_decode_pos(d, g, p);
#pragma unroll
        for (int k = 0; k < NCO_T; ++k) {
            const int col = cg + 8 * k;
            s_g[pi * RG + col] = valid ? wgrad_load_g(wd, g, ps, co0 + col) : 0.f;
        }
#pragma unroll
        for (int i = 0; i < NCOL_T; ++i) s_v[pi * WG_ROW_V + cg + 8 * i] = valid ? wgrad_load_v(d, g, ps, cols[i]) : 0.f;
        __syncthreads();
#pragma unroll
        for (int k2 = 0; k2 < WG_KP / 2; ++k2) {
            const int kk = 2 * k2 + khalf;
            const float b = s_v[kk * WG_ROW_V + wave * 32 + l31];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const float a = s_g[kk * RG + m * 32 + l31];
                acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[m], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    const int j = col0 + wave * 32 + l31;
    if (j >= g.ncol) return;
    float* out = wd.work + (int64_t)slab * d.cout * g.ncol + j;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + m * 32 + wgrad_mfma_row(r, lane);
            if (co < d.cout) out[(int64_t)co * g.ncol] = acc[m][r];
        }
}

__global__ __launch_bounds__(256) void conv_wgrad_reduce_kernel(const sda_wgrad_desc wd, const WgradGeom g) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < (int64_t)wd.conv.cout * g.ncol) wgrad_reduce_one(wd, g, e);
}

template <int MT>
static int wgrad_launch_t(const sda_wgrad_desc* d, const WgradGeom& g, hipStream_t stream) {
    hipLaunchKernelGGL(conv_wgrad_kernel<MT>, dim3(g.grid), dim3(WG_THREADS), 0, stream, *d, g);
    return sda_launch_status();
}

extern "C" int sda_conv_wgrad(const sda_wgrad_desc* d, void* stream) {
    WgradGeom g;
    int rc = wgrad_plan(d, &g);
    if (rc != SDA_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    switch (g.mt) {
        case 1: rc = wgrad_launch_t<1>(d, g, st); break;
        case 2: rc = wgrad_launch_t<2>(d, g, st); break;
        case 3: rc = wgrad_launch_t<3>(d, g, st); break;
        default: rc = wgrad_launch_t<4>(d, g, st); break;
    }
    if (rc != SDA_OK) return rc;
    const int64_t total = (int64_t)d->conv.cout * g.ncol;
    hipLaunchKernelGGL(conv_wgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, *d, g);
    return sda_launch_status();
}

// ---------------------------------------------------------------- modulation gradient: planar spatial sums
// out[i * out_sn + ch] (+)= sum_{pix} (x - y)[i][ch][pix]   (y optional), or with sum_images: out[ch] (+)= sum_i sum_pix.
// One workgroup per output element; each thread strides through the plane(s), then a fixed-order tree in LDS.
__global__ __launch_bounds__(256) void plane_sum_kernel(const float* __restrict__ x, const float* __restrict__ y, int n, int c,
                                                        int64_t hw, float* out, int64_t out_sn, int sum_images, int accumulate) {
    __shared__ float red[256];
    const int ch = blockIdx.x % c;
    const int i0 = sum_images ? 0 : blockIdx.x / c;
    const int i1 = sum_images ? n : i0 + 1;
    float s = 0.f;
    for (int i = i0; i < i1; ++i) {
        const int64_t base = ((int64_t)i * c + ch) * hw;
        for (int64_t k = threadIdx.x; k < hw; k += 256) s += y ? x[base + k] - y[base + k] : x[base + k];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float* o = out + (int64_t)i0 * out_sn + ch;
        *o = accumulate ? *o + red[0] : red[0];
    }
}

extern "C" int sda_plane_sum(const float* x, const float* y, int n, int c, int64_t hw, float* out, int64_t out_sn, int sum_images,
                             int accumulate, void* stream) {
    if (!x || !out || n <= 0 || c <= 0 || hw <= 0) return SDA_E_BADARG;
    const int64_t blocks = sum_images ? (int64_t)c : (int64_t)n * c;
    if (blocks > 0x7fffffffL) return SDA_E_UNSUPPORTED;
    hipLaunchKernelGGL(plane_sum_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, y, n, c, hw, out, out_sn,
                       sum_images, accumulate);
    return sda_launch_status();
}

#endif  // !SDA_HOST_EMU

// planning entries (host only: nothing is launched)
extern "C" int sda_conv_wgrad_slabs(const sda_wgrad_desc* d) {
    WgradGeom g;
    int rc = wgrad_plan(d, &g);
    return rc != SDA_OK ? rc : g.slabs;
}

extern "C" int64_t sda_conv_wgrad_work_floats(const sda_wgrad_desc* d) {
    WgradGeom g;
    int rc = wgrad_plan(d, &g);
    return rc != SDA_OK ? (int64_t)rc : (int64_t)g.slabs * d->conv.cout * g.ncol;
}

// ---------------------------------------------------------------- CPU emulator (tests only; libsda_emu.so)
#ifdef SDA_HOST_EMU
#include <vector>
// Replays conv_wgrad_kernel<MT> + conv_wgrad_reduce_kernel on the host with HOST pointers (d->work included): same planner,
// same staging maps, same MFMA lane maps (A[i=l&31][k=l>>5], B[k=l>>5][j=l&31], D row = wgrad_mfma_row(r,l), col = l&31) in
// the same k order, same slab-ordered reduction.
extern "C" int sda_conv_wgrad_emulate(const sda_wgrad_desc* dp) {
    WgradGeom g;
    int rc = wgrad_plan(dp, &g);
    if (rc != SDA_OK) return rc;
    const sda_wgrad_desc& wd = *dp;
    const sda_conv_desc& d = wd.conv;
    const int BM = g.bm, MT = g.mt, RG = WG_ROW_G(BM);
    std::vector<float> s_g((size_t)WG_KP * RG), s_v((size_t)WG_KP * WG_ROW_V), acc((size_t)WG_THREADS * MT * 16);
    for (int b = 0; b < g.grid; ++b) {
        int slab, ct, colt;
        wgrad_decode_block(g, b, slab, ct, colt);
        const int co0 = ct * BM, col0 = colt * WG_BN;
        std::fill(acc.begin(), acc.end(), 0.f);
        const int64_t p_begin = (int64_t)slab * g.per;
        const int64_t p_end = p_begin + g.per < g.P ? p_begin + g.per : g.P;
        for (int64_t p0 = p_begin; p0 < p_end; p0 += WG_KP) {
            for (int tid = 0; tid < WG_THREADS; ++tid) {
                const int pi = tid & (WG_KP - 1), cg = tid / WG_KP;
                const int64_t p = p0 + pi;
                const bool valid = p < p_end;
                WgradPos ps;
                ps.n = 0; ps.oy = 0; ps.ox = 0;
                if (valid) ps = wgrad_decode_pos(d, g, p);
                for (int k = 0; k < BM / 8; ++k) {
                    const int col = cg + 8 * k;
                    s_g[(size_t)pi * RG + col] = valid ? wgrad_load_g(wd, g, ps, co0 + col) : 0.f;
                }
                for (int i = 0; i < WG_BN / 8; ++i)
                    s_v[(size_t)pi * WG_ROW_V + cg + 8 * i] = valid ? wgrad_load_v(d, g, ps, wgrad_decode_col(d, g, col0 + cg + 8 * i)) : 0.f;
            }
            for (int wave = 0; wave < 4; ++wave)
                for (int k2 = 0; k2 < WG_KP / 2; ++k2)
                    for (int m = 0; m < MT; ++m) {
                        float A[32][2], B[2][32];
                        for (int lane = 0; lane < 64; ++lane) {
                            const int l31 = lane & 31, kh_ = lane >> 5, kk = 2 * k2 + kh_;
                            B[kh_][l31] = s_v[(size_t)kk * WG_ROW_V + wave * 32 + l31];
                            A[l31][kh_] = s_g[(size_t)kk * RG + m * 32 + l31];
                        }
                        for (int lane = 0; lane < 64; ++lane)
                            for (int r = 0; r < 16; ++r) {
                                const int i = wgrad_mfma_row(r, lane), jj = lane & 31;
                                float& c = acc[((size_t)(wave * 64 + lane) * MT + m) * 16 + r];
                                c = fmaf(A[i][0], B[0][jj], c);
                                c = fmaf(A[i][1], B[1][jj], c);
                            }
                    }
        }
        for (int tid = 0; tid < WG_THREADS; ++tid) {
            const int lane = tid & 63, wave = tid >> 6;
            const int j = col0 + wave * 32 + (lane & 31);
            if (j >= g.ncol) continue;
            for (int m = 0; m < MT; ++m)
                for (int r = 0; r < 16; ++r) {
                    const int co = co0 + m * 32 + wgrad_mfma_row(r, lane);
                    if (co < d.cout) wd.work[((int64_t)slab * d.cout + co) * g.ncol + j] = acc[((size_t)tid * MT + m) * 16 + r];
                }
        }
    }
    const int64_t total = (int64_t)d.cout * g.ncol;
    for (int64_t e = 0; e < total; ++e) wgrad_reduce_one(wd, g, e);
    return SDA_OK;
}
#endif  // SDA_HOST_EMU
