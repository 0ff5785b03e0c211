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
#include "conv_wgrad.hpp"


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

int wgrad_launch_reduce(const sda_wgrad_desc* d, const WgradGeom& g, hipStream_t stream) {
    const int64_t total = (int64_t)d->conv.cout * g.ncol;
    hipLaunchKernelGGL(conv_wgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, *d, g);
    return sda_launch_status();
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
    return wgrad_launch_reduce(d, g, st);
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
