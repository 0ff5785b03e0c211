// Parameter gradients of a whole residual MLP (the Lorenz LOCAL score kernel; opt-in training, sda_amd/training.py with mlp = True).
// A training step of the reference's train_local is 64 rows through 12 GEMMs of at most 256 x 256: bound by launch latency, so the
// backward is THREE launches on top of the forward's, whatever the depth:
//   1. sda_mlp_bwd_train: the input VJP of the chain, the kernel text of sda_mlp_bwd (csrc/mlp1d_vjp_kernels.hpp, included by csrc/mlp1d.hip
//      and by this file: same slabs, same saves, the same input gradient bit for bit; one wave per 16 rows, one wave per SIMD) that also stores the
//      cotangent at every GEMM's output as rows g_save[gemm][row][g_ld]: the cotangent of a Linear's / a block's output (kinds 0, 2) behind
//      that GEMM's multiply, gz = (g W2) * act'(z) (kind 1) behind the activation derivative.  The stores leave behind the hand-off
//      barrier, as the forward's saves do (in front of the staging loads a store's round trip is what the wait for those loads waits for);
//   2. sda_mlp_wgrad: ONE launch for all GEMMs, dW[o][i] = sum_r G[r][o] U[r][i] with the bias as one more column (U = 1), an implicit
//      GEMM per layer with M = out_f, N = in_f + 1 and the contraction over the rows -- conv_wgrad.hip's discipline: the row axis is cut into
//      `slabs` contiguous ranges (a function of the shapes only); workgroup (slab, GEMM, out tile, column tile) owns a 64 x 128 tile of
//      one GEMM's result over its slab and writes it, unreduced, to work; per stage of 32 rows it stages G[32][64] and U[32][128] into
//      LDS (U rebuilt from what the forward saved: a Linear's input rows, (a - mean) rstd, act(z) -- nothing is materialised), then each of
//      the 4 waves issues v_mfma_f32_32x32x2_f32 over its 32 columns;
//   3. the slab reduction: sums the slabs in slab order (no atomics anywhere: bitwise reproducible) and writes or adds dW, db in torch's
//      unpadded [out][in] / [out] layout.
// Index arithmetic of 2 and 3 is in __host__ __device__ helpers; the emulator at the bottom (libsda_emu.so, tests only) replays the
// planner, the staging maps, the MFMA lane maps and the reduction order on the CPU.
#ifndef SDA_HOST_EMU
#include "mlp1d_common.hpp"
#else
#include "sda_common.hpp"
#endif

// ------------------------------------------------------------------------------------------------------------ weight gradient: plan
#define MW_THREADS 256
#define MW_KP 32                 // rows per stage
#define MW_BM 64                 // output features per workgroup (two 32-row MFMA tiles)
#define MW_BN 128                // columns per workgroup (4 waves x 32)
#define MW_MAX_SLABS 64
#define MW_TARGET_BLOCKS 1024    // enough workgroups to fill 256 CUs four times over
#define MW_ROW_G (MW_BM + 1)     // LDS row pitch (floats) of the staged cotangent
#define MW_ROW_U (MW_BN + 1)     // ... and of the staged input

struct MwGeom {
    int slabs;
    int per;                              // rows per slab (a multiple of MW_KP)
    int tiles;                            // (out tile, column tile) pairs of all GEMMs
    int grid;                             // tiles * slabs
    int elems;                            // sum of out_f (in_f + 1)
    int tile0[SDA_MLP_MAXG + 1];          // first tile of GEMM g
    int elem0[SDA_MLP_MAXG + 1];          // first element of GEMM g in a slab of work: work[slab * elems + elem0[g] + o (in_f + 1) + j]
};

__host__ __device__ inline int mw_ncol(int in_f) { return in_f + 1; }
__host__ __device__ inline int mw_n_ct(int out_f) { return (out_f + MW_BM - 1) / MW_BM; }
__host__ __device__ inline int mw_n_colt(int in_f) { return (mw_ncol(in_f) + MW_BN - 1) / MW_BN; }

// need_work: a launch (or the replay) needs d->work; the planning entries size that buffer, so they do not ask for it
static int mw_plan(const sda_mlp_wgrad_desc* d, MwGeom* g, bool need_work) {
    if (!d || d->rows < 1 || d->ngemm < 1 || d->ngemm > SDA_MLP_MAXG) return SDA_E_UNSUPPORTED;
    if (need_work && !d->work) return SDA_E_BADARG;
    if (d->slabs < 0 || d->slabs > MW_MAX_SLABS) return SDA_E_BADARG;
    g->tile0[0] = 0; g->elem0[0] = 0;
    for (int k = 0; k < d->ngemm; ++k) {
        const int in_f = d->in_f[k], out_f = d->out_f[k];
        if (in_f < 1 || out_f < 1 || in_f > 256 || out_f > 256 || d->kind[k] < 0 || d->kind[k] > 2) return SDA_E_UNSUPPORTED;
        if (!d->src[k] || !d->g[k] || !d->dw[k]) return SDA_E_BADARG;
        if (d->kind[k] == 1 && (!d->mean[k] || !d->rstd[k])) return SDA_E_BADARG;
        if (d->src_ld[k] < in_f || d->g_ld < out_f) return SDA_E_BADARG;
        g->tile0[k + 1] = g->tile0[k] + mw_n_ct(out_f) * mw_n_colt(in_f);
        g->elem0[k + 1] = g->elem0[k] + out_f * mw_ncol(in_f);
    }
    g->tiles = g->tile0[d->ngemm];
    g->elems = g->elem0[d->ngemm];
    const int stages = (d->rows + MW_KP - 1) / MW_KP;
    int s = d->slabs;
    if (s == 0) {                                            // the planner's choice: a function of the shapes only
        s = (MW_TARGET_BLOCKS + g->tiles - 1) / g->tiles;
        if (s > MW_MAX_SLABS) s = MW_MAX_SLABS;
    }
    if (s > stages) s = stages;
    if (s < 1) s = 1;
    g->per = (stages + s - 1) / s * MW_KP;
    g->slabs = (d->rows + g->per - 1) / g->per;              // (no empty slab)
    g->grid = g->tiles * g->slabs;
    return SDA_OK;
}

// ---------------------------------------------------------------- index helpers (host + device)

// D-fragment row of accumulator register r for v_mfma_f32_32x32x2_f32 (col = lane & 31)
__host__ __device__ inline int mw_mfma_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// workgroup b -> (slab, GEMM, out tile, column tile)
__host__ __device__ inline void mw_decode_block(const sda_mlp_wgrad_desc& d, const MwGeom& g, int b, int& slab, int& gemm, int& ct, int& colt) {
    slab = b / g.tiles;
    const int t = b - slab * g.tiles;
    gemm = 0;
    while (gemm + 1 < d.ngemm && t >= g.tile0[gemm + 1]) ++gemm;
    const int local = t - g.tile0[gemm], nc = mw_n_colt(d.in_f[gemm]);
    ct = local / nc;
    colt = local - ct * nc;
}

// staging maps: element e of a stage's G tile [MW_KP rows][MW_BM features] / U tile [MW_KP rows][MW_BN columns] -> (row of the stage, column);
// thread tid stages elements tid + MW_THREADS i: consecutive threads read consecutive features of a row
__host__ __device__ inline void mw_stage_g(int e, int& r, int& col) { r = e / MW_BM; col = e - r * MW_BM; }
__host__ __device__ inline void mw_stage_u(int e, int& r, int& col) { r = e / MW_BN; col = e - r * MW_BN; }

__host__ __device__ inline float mw_load_g(const sda_mlp_wgrad_desc& d, int gemm, int64_t row, int o) {
    return o < d.out_f[gemm] ? d.g[gemm][row * d.g_ld + o] : 0.f;
}
// column j of the multiply's second operand for `row`: U[row][j] for j < in_f, the constant 1 (the bias column) for j == in_f, 0 beyond
__host__ __device__ inline float mw_load_u(const sda_mlp_wgrad_desc& d, int gemm, int64_t row, int j) {
    const int in_f = d.in_f[gemm];
    if (j >= in_f) return j == in_f ? 1.f : 0.f;
    const float v = d.src[gemm][row * d.src_ld[gemm] + j];
    if (d.kind[gemm] == 1) return (v - d.mean[gemm][row]) * d.rstd[gemm][row];     // (the forward's order: (a - mean), then x rstd)
    if (d.kind[gemm] == 2) return sda_act(d.act, v);
    return v;
}

// reduction of element e (of one slab's `elems`) over the slabs, in slab order
__host__ __device__ inline void mw_reduce_one(const sda_mlp_wgrad_desc& d, const MwGeom& g, int e) {
    float s = 0.f;
    for (int k = 0; k < g.slabs; ++k) s += d.work[(int64_t)k * g.elems + e];
    int gemm = 0;
    while (gemm + 1 < d.ngemm && e >= g.elem0[gemm + 1]) ++gemm;
    const int local = e - g.elem0[gemm], ncol = mw_ncol(d.in_f[gemm]);
    const int o = local / ncol, j = local - o * ncol;
    float* out = nullptr;
    if (j < ncol - 1) out = d.dw[gemm] + (int64_t)o * (ncol - 1) + j;
    else if (d.db[gemm]) out = d.db[gemm] + o;
    if (out) *out = d.accumulate ? *out + s : s;
}

// ------------------------------------------------------------------------------------------------------------ the kernels
#ifndef SDA_HOST_EMU

typedef float mw_f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(MW_THREADS) void mlp_wgrad_kernel(const sda_mlp_wgrad_desc d, const MwGeom g) {
    constexpr int MT = MW_BM / 32;
    __shared__ float s_g[MW_KP * MW_ROW_G];
    __shared__ float s_u[MW_KP * MW_ROW_U];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, khalf = lane >> 5;
    int slab, gemm, ct, colt;
    mw_decode_block(d, g, blockIdx.x, slab, gemm, ct, colt);
    const int o0 = ct * MW_BM, col0 = colt * MW_BN;
    const int out_f = d.out_f[gemm], ncol = mw_ncol(d.in_f[gemm]);

    mw_f32x16 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;

    const int r_begin = slab * g.per;
    const int r_end = r_begin + g.per < d.rows ? r_begin + g.per : d.rows;
    for (int r0 = r_begin; r0 < r_end; r0 += MW_KP) {
#pragma unroll
        for (int i = 0; i < MW_KP * MW_BM / MW_THREADS; ++i) {
            int r, col;
            mw_stage_g(tid + MW_THREADS * i, r, col);
            s_g[r * MW_ROW_G + col] = r0 + r < r_end ? mw_load_g(d, gemm, r0 + r, o0 + col) : 0.f;
        }
#pragma unroll
        for (int i = 0; i < MW_KP * MW_BN / MW_THREADS; ++i) {
            int r, col;
            mw_stage_u(tid + MW_THREADS * i, r, col);
            s_u[r * MW_ROW_U + col] = r0 + r < r_end ? mw_load_u(d, gemm, r0 + r, col0 + col) : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k2 = 0; k2 < MW_KP / 2; ++k2) {
            const int kk = 2 * k2 + khalf;
            const float b = s_u[kk * MW_ROW_U + wave * 32 + l31];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const float a = s_g[kk * MW_ROW_G + m * 32 + l31];
                acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[m], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    const int j = col0 + wave * 32 + l31;
    if (j >= ncol) return;
    float* out = d.work + (int64_t)slab * g.elems + g.elem0[gemm] + j;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = o0 + m * 32 + mw_mfma_row(r, lane);
            if (o < out_f) out[(int64_t)o * ncol] = acc[m][r];
        }
}

__global__ __launch_bounds__(256) void mlp_wgrad_reduce_kernel(const sda_mlp_wgrad_desc d, const MwGeom g) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < g.elems) mw_reduce_one(d, g, e);
}

extern "C" int sda_mlp_wgrad(const sda_mlp_wgrad_desc* d, void* stream) {
    MwGeom g;
    const int rc = mw_plan(d, &g, true);
    if (rc != SDA_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mlp_wgrad_kernel, dim3(g.grid), dim3(MW_THREADS), 0, st, *d, g);
    const int lr = sda_launch_status();
    if (lr != SDA_OK) return lr;
    hipLaunchKernelGGL(mlp_wgrad_reduce_kernel, dim3((g.elems + 255) / 256), dim3(256), 0, st, *d, g);
    return sda_launch_status();
}

// ------------------------------------------------------------------------------------------------------------ VJP + cotangent streams
// the wave's rows of the cotangent at GEMM g's output -> g_save[g][row][..]: whole fragments (zeros beyond the width, see sda_hip.h)
template <int NF>
__device__ __forceinline__ void mt_store_cot(const sda_mlp_train_desc& t, int g, int width, const MlCtx& c, const ml_f32x4 (&v)[NF]) {
    if (!c.rowok) return;
    float* o = t.g_save + (int64_t)g * t.g_stride + c.row * t.g_ld + 4 * c.kq;
    const int nm = NF == 8 ? ml_mf(width) : mlw_mf(width);
#pragma unroll
    for (int m = 0; m < NF; ++m)
        if (m < nm) *reinterpret_cast<ml_f32x4*>(o + 16 * m) = v[m];
}

// The two VJP kernels are the text of mlp_bwd_kernel / mlp_bwd_kernel_wide (csrc/mlp1d_vjp_kernels.hpp, which csrc/mlp1d.hip includes too),
// compiled here under names of this unit's own with the descriptor pair as the parameter and the cotangent hook filled in.  Only <false>
// (rows, not windows) is instantiated: `w` exists so that the discarded window branches parse (not const: the compiler would fold its zeros
// into that text and warn of a division by w.c).
#define ML_VJP_ARGS const sda_mlp_train_desc t
#define ML_VJP_ENTRY const sda_mlp_desc& d = t.mlp; sda_mlp_win w = {};
#define ML_COT(g, n, v) mt_store_cot(t, (g), (n), c, v)
#define ML_WF 1
#define ML_K_BWD mlp_train_vjp_kernel
#define ML_K_BWD_WIDE mlp_train_vjp_kernel_wide
#include "mlp1d_vjp_kernels.hpp"

extern "C" int sda_mlp_bwd_train(const sda_mlp_train_desc* t, void* stream) {
    if (!t) return SDA_E_BADARG;
    const sda_mlp_desc* d = &t->mlp;
    bool wide = false;
    const int rc = mlp_check(d, true, false, &wide);
    if (rc != SDA_OK) return rc;
    int wpad = 16;                                         // the widest padded GEMM output: what a row of g_save must hold
    for (int g = 0; g < d->ngemm; ++g) {
        const int p = 16 * (wide ? mlw_mf(d->out_f[g]) : ml_mf(d->out_f[g]));
        if (p > wpad) wpad = p;
    }
    if (!t->g_save || (reinterpret_cast<uintptr_t>(t->g_save) & 15) || t->g_ld < wpad || (t->g_ld & 3) || (t->g_stride & 3) ||
        t->g_stride < (int64_t)d->rows * t->g_ld)
        return SDA_E_BADARG;
    const int64_t tiles = ((int64_t)d->rows + 63) / 64;
    if (tiles > 0x7fffffffLL) return SDA_E_UNSUPPORTED;
    constexpr int lds = (2 * ML_SLAB + ML_BIAS) * 4;
    static bool raised[2][SDA_MAX_DEVICES];
    void (*const kern)(sda_mlp_train_desc) = wide ? mlp_train_vjp_kernel_wide<false> : mlp_train_vjp_kernel<false>;
    const int rr = sda_raise_dyn_lds(reinterpret_cast<const void*>(kern), lds, raised[wide]);
    if (rr != SDA_OK) return rr;
    hipLaunchKernelGGL(kern, dim3((unsigned)tiles), dim3(256), lds, (hipStream_t)stream, *t);
    return sda_launch_status();
}

#endif  // !SDA_HOST_EMU

// planning entries (host only: nothing is launched)
extern "C" int sda_mlp_wgrad_slabs(const sda_mlp_wgrad_desc* d) {
    MwGeom g;
    const int rc = mw_plan(d, &g, false);
    return rc != SDA_OK ? rc : g.slabs;
}

extern "C" int64_t sda_mlp_wgrad_work_floats(const sda_mlp_wgrad_desc* d) {
    MwGeom g;
    const int rc = mw_plan(d, &g, false);
    return rc != SDA_OK ? (int64_t)rc : (int64_t)g.slabs * g.elems;
}

// ------------------------------------------------------------------------------------------------------------ CPU emulator (tests only; libsda_emu.so)
#ifdef SDA_HOST_EMU
#include <algorithm>
#include <vector>
// Replays mlp_wgrad_kernel + mlp_wgrad_reduce_kernel on the host with HOST pointers (d->work included): same planner, same block decode,
// same staging maps, same MFMA lane maps (A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31], D row = mw_mfma_row(r, l), col = l & 31)
// in the same k order, same slab-ordered reduction.
extern "C" int sda_mlp_wgrad_emulate(const sda_mlp_wgrad_desc* dp) {
    MwGeom g;
    const int rc = mw_plan(dp, &g, true);
    if (rc != SDA_OK) return rc;
    const sda_mlp_wgrad_desc& d = *dp;
    constexpr int MT = MW_BM / 32;
    std::vector<float> s_g((size_t)MW_KP * MW_ROW_G), s_u((size_t)MW_KP * MW_ROW_U), acc((size_t)MW_THREADS * MT * 16);
    for (int b = 0; b < g.grid; ++b) {
        int slab, gemm, ct, colt;
        mw_decode_block(d, g, b, slab, gemm, ct, colt);
        const int o0 = ct * MW_BM, col0 = colt * MW_BN;
        const int out_f = d.out_f[gemm], ncol = mw_ncol(d.in_f[gemm]);
        std::fill(acc.begin(), acc.end(), 0.f);
        const int r_begin = slab * g.per;
        const int r_end = r_begin + g.per < d.rows ? r_begin + g.per : d.rows;
        for (int r0 = r_begin; r0 < r_end; r0 += MW_KP) {
            for (int tid = 0; tid < MW_THREADS; ++tid) {
                for (int i = 0; i < MW_KP * MW_BM / MW_THREADS; ++i) {
                    int r, col;
                    mw_stage_g(tid + MW_THREADS * i, r, col);
                    s_g[(size_t)r * MW_ROW_G + col] = r0 + r < r_end ? mw_load_g(d, gemm, r0 + r, o0 + col) : 0.f;
                }
                for (int i = 0; i < MW_KP * MW_BN / MW_THREADS; ++i) {
                    int r, col;
                    mw_stage_u(tid + MW_THREADS * i, r, col);
                    s_u[(size_t)r * MW_ROW_U + col] = r0 + r < r_end ? mw_load_u(d, gemm, r0 + r, col0 + col) : 0.f;
                }
            }
            for (int wave = 0; wave < 4; ++wave)
                for (int k2 = 0; k2 < MW_KP / 2; ++k2)
                    for (int m = 0; m < MT; ++m) {
                        float A[32][2], B[2][32];
                        for (int lane = 0; lane < 64; ++lane) {
                            const int l31 = lane & 31, kh_ = lane >> 5, kk = 2 * k2 + kh_;
                            B[kh_][l31] = s_u[(size_t)kk * MW_ROW_U + wave * 32 + l31];
                            A[l31][kh_] = s_g[(size_t)kk * MW_ROW_G + m * 32 + l31];
                        }
                        for (int lane = 0; lane < 64; ++lane)
                            for (int r = 0; r < 16; ++r) {
                                const int i = mw_mfma_row(r, lane), jj = lane & 31;
                                float& cv = acc[((size_t)(wave * 64 + lane) * MT + m) * 16 + r];
                                cv = fmaf(A[i][0], B[0][jj], cv);
                                cv = fmaf(A[i][1], B[1][jj], cv);
                            }
                    }
        }
        for (int tid = 0; tid < MW_THREADS; ++tid) {
            const int lane = tid & 63, wave = tid >> 6;
            const int j = col0 + wave * 32 + (lane & 31);
            if (j >= ncol) continue;
            for (int m = 0; m < MT; ++m)
                for (int r = 0; r < 16; ++r) {
                    const int o = o0 + m * 32 + mw_mfma_row(r, lane);
                    if (o < out_f) d.work[(int64_t)slab * g.elems + g.elem0[gemm] + (int64_t)o * ncol + j] = acc[((size_t)tid * MT + m) * 16 + r];
                }
        }
    }
    for (int e = 0; e < g.elems; ++e) mw_reduce_one(d, g, e);
    return SDA_OK;
}
#endif  // SDA_HOST_EMU
