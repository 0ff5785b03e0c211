// Domain-localised form of the ensemble-space Kalman smoother (enks_wide.hip is the global form): the state is a periodic grid
// (C, Hg, Wg) cut into blocks of bh x bw points, and every block solves its own M x M system over the observed values near it,
// each weighted by a Gaspari-Cohn factor rho (R-localisation).  The lists (per block: which observed values, with which rho) are
// built ONCE on the host in float64 and handed in as a CSR plan; prepare and inflation are enks_wide.hip's, unchanged.  Per
// analysis THREE launches after sda_enkw_prepare:
//   sda_enkl_pack       T[i] = (Y[:, i] | D[:, i]): an observed value becomes 2 M contiguous floats     a 32 x 32 LDS transpose
//   sda_enkl_weights    per block [G_b | B_b] over its list, Cholesky, W[b] (fp32), status[b]           v_mfma_f64_16x16x4_f64
//   sda_enkl_transform  x_j += sum_m W[b][m][j] (x_m - xbar) on every block, tile and slab              v_mfma_f32_16x16x4_f32
// (include/sda_hip.h states the arithmetic; DESIGN.md section 5.2e-3 the reasons.)  A workgroup owns its block from the first load
// to the last store: no atomics, no workgroup waits for another, every sum has an order fixed by the list and M, so results are
// bitwise reproducible, a block's result depends on its own list alone, and a slab's on M, the block and W[b] alone.
//
// Under SDA_HOST_EMU the same arithmetic in the same summation orders runs as plain loops over host arrays (bottom of the file).
#include "sda_common.hpp"

#include <math.h>

#define ENKL_MAX_M 128              // L[M][M] float64 in LDS: 128 KiB of the 160 KiB (enks_wide.hip's cap)
#define ENKL_MAX_K (1 << 24)
#define ENKL_TC 128                 // block components per transform tile
#define ENKL_LD (ENKL_TC + 16)      // LDS row stride of the tile: rows m .. m + 3 of one B operand fall on 64 distinct banks
#define ENKL_THREADS 256
#define ENKL_MAX_THREADS 1024
#define ENKL_MAX_SLABS 65535
#define ENKL_MAX_BLOCKS (1 << 22)

__host__ __device__ static inline int enkl_pad16(int m) { return (m + 15) & ~15; }

static int enkl_shape_check(int m, int k) {
    if (m < 1 || k < 1) return SDA_E_BADARG;
    if (m < 2 || m > ENKL_MAX_M || k > ENKL_MAX_K) return SDA_E_UNSUPPORTED;
    return SDA_OK;
}

static int enkl_pack_check(const float* Y, const float* D, int m, int k, const float* T) {
    if (!Y || !D || !T) return SDA_E_BADARG;
    return enkl_shape_check(m, k);
}

static int enkl_weights_check(const float* T, int m, int k, const int32_t* offsets, const int32_t* idx, const float* rho, int nblk,
                              float sigma, const double* bwork, const float* W, const int32_t* status) {
    if (!T || !offsets || !idx || !rho || !bwork || !W || !status || nblk < 1 || !(sigma > 0.f)) return SDA_E_BADARG;
    if (nblk > ENKL_MAX_BLOCKS) return SDA_E_UNSUPPORTED;
    return enkl_shape_check(m, k);
}

static int enkl_transform_check(const float* S, int64_t s_st, int64_t s_sp, int nslab, int m, int C, int Hg, int Wg, int bh, int bw,
                                const int32_t* offsets, const float* W) {
    if (!S || !offsets || !W || nslab < 1 || m < 1 || C < 1 || Hg < 1 || Wg < 1 || bh < 1 || bw < 1 || s_st < 0) return SDA_E_BADARG;
    if (Hg % bh != 0 || Wg % bw != 0 || s_sp < (int64_t)C * Hg * Wg) return SDA_E_BADARG;
    const int64_t nblk = (int64_t)(Hg / bh) * (Wg / bw), nb = (int64_t)C * bh * bw;
    if (m < 2 || m > ENKL_MAX_M || nslab > ENKL_MAX_SLABS || nblk > ENKL_MAX_BLOCKS || nb > ((int64_t)1 << 30) ||
        nblk * ((nb + ENKL_TC - 1) / ENKL_TC) > 0x7fffffff)
        return SDA_E_UNSUPPORTED;
    return SDA_OK;
}

// component q of block (br, bc): channel q / (bh bw), then row-major inside the block; its offset inside a member's state
__host__ __device__ static inline int64_t enkl_offset(int64_t q, int br, int bc, int Hg, int Wg, int bh, int bw) {
    const int64_t ch = q / (bh * bw);
    const int rem = (int)(q % (bh * bw));
    return (ch * Hg + (int64_t)br * bh + rem / bw) * Wg + (int64_t)bc * bw + rem % bw;
}

#ifndef SDA_HOST_EMU
typedef double enkl_d4 __attribute__((ext_vector_type(4)));
typedef float enkl_f4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- pack: grid (tiles of 32 observed values, tiles of 32 of the 2 M rows)
__global__ __launch_bounds__(ENKL_THREADS) void enkl_pack_kernel(const float* __restrict__ Y, const float* __restrict__ D, int m, int k,
                                                                 float* __restrict__ T) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int i0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int r = ty; r < 32; r += ENKL_THREADS / 32) {
        const int row = r0 + r, i = i0 + tx;
        float v = 0.f;
        if (row < 2 * m && i < k) v = row < m ? Y[(int64_t)row * k + i] : D[(int64_t)(row - m) * k + i];
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += ENKL_THREADS / 32) {
        const int i = i0 + r, row = r0 + tx;
        if (i < k && row < 2 * m) T[(int64_t)i * 2 * m + row] = tile[tx][r];
    }
}

extern "C" int sda_enkl_pack(const float* Y, const float* D, int m, int k, float* T, void* stream) {
    int rc = enkl_pack_check(Y, D, m, k, T);
    if (rc != SDA_OK) return rc;
    hipLaunchKernelGGL(enkl_pack_kernel, dim3((unsigned)((k + 31) / 32), (unsigned)((2 * m + 31) / 32)), dim3(ENKL_THREADS), 0,
                       (hipStream_t)stream, Y, D, m, k, T);
    return sda_launch_status();
}

// ---------------------------------------------------------------- weights: ONE workgroup per block, 256 .. 1024 threads by M.
// LDS (dynamic): L[m][m] doubles, one flag.  The waves share the 16 x 16 tiles of [G_b | B_b] round-robin; a tile is one accumulator
// chained over the block's list in list order, 4 observed values per float64 MFMA: lane l holds row (l & 15) of its tile at value
// (l >> 4) for both operands (an NT product), the A operand already times rho (exact in float64).  Rows past M and values past the
// list enter as zeros.  G_b lands in L, B_b in this block's m x m doubles of bwork; then enkw_solve_kernel's factor and solve.
__global__ __launch_bounds__(ENKL_MAX_THREADS) void enkl_weights_kernel(const float* __restrict__ T, int m, int k,
                                                                        const int32_t* __restrict__ offsets,
                                                                        const int32_t* __restrict__ idx, const float* __restrict__ rho,
                                                                        float sigma, double* __restrict__ bwork, float* __restrict__ W,
                                                                        int32_t* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char enkl_smem[];
    double* L = (double*)enkl_smem;
    int* bad = (int*)(L + m * m);
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int b = blockIdx.x;
    const int lo = offsets[b], n = offsets[b + 1] - lo;
    float* Wb = W + (int64_t)b * m * m;
    double* bw = bwork + (int64_t)b * m * m;
    if (n <= 0) {                                            // an empty list: W_b = 0 (workgroup-uniform; no barrier was passed)
        for (int e = tid; e < m * m; e += nthr) Wb[e] = 0.f;
        if (tid == 0) status[b] = 0;
        return;
    }
    if (tid == 0) *bad = 0;
    const int mp = enkl_pad16(m), rt = mp >> 4;
    const int lane = tid & 63, wave = tid >> 6, nwave = nthr >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const double s2 = (double)sigma * (double)sigma;
    bool stray = false;
    for (int tile = wave; tile < rt * 2 * rt; tile += nwave) {                     // wave-uniform
        const int ti = tile / (2 * rt), ct = tile % (2 * rt);
        const int row = ti * 16 + r16;
        const int col = (ct < rt ? ct : ct - rt) * 16 + r16;
        const bool a_ok = row < m, b_ok = col < m;
        const int boff = (ct < rt ? 0 : m) + col;
        enkl_d4 acc = enkl_d4{0.0, 0.0, 0.0, 0.0};
        for (int c0 = 0; c0 < n; c0 += 4) {
            const int c = c0 + kq;
            double a = 0.0, bv = 0.0;
            if (c < n) {
                const int ix = idx[lo + c];
                if ((unsigned)ix < (unsigned)k) {
                    const float* t = T + (int64_t)ix * 2 * m;
                    if (a_ok) a = (double)rho[lo + c] * (double)t[row];
                    if (b_ok) bv = (double)t[boff];
                } else {
                    stray = true;                            // an index outside the observed values: not read, the block is flagged
                }
            }
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = ti * 16 + kq + 4 * r;
            if (i < m && col < m) {
                const double v = acc[r] / (double)(m - 1);
                if (ct < rt) L[i * m + col] = v + (i == col ? s2 : 0.0);
                else bw[i * m + col] = v;
            }
        }
    }
    __syncthreads();
    if (stray) *bad = 1;                                     // every writer stores the same value
    // Cholesky, right-looking, in the lower triangle of L
    for (int p = 0; p < m; ++p) {
        if (tid == 0) {
            double v = L[p * m + p];
            if (!(v > 0.0) || !(v < INFINITY)) { *bad = 1; v = 1.0; }
            L[p * m + p] = sqrt(v);
        }
        __syncthreads();
        const double piv = L[p * m + p];
        for (int i = p + 1 + tid; i < m; i += nthr) L[i * m + p] = L[i * m + p] / piv;
        __syncthreads();
        const int nn = m - p - 1;
        for (int e = tid; e < nn * nn; e += nthr) {
            const int i = p + 1 + e / nn, c = p + 1 + e % nn;
            if (c <= i) L[i * m + c] -= L[i * m + p] * L[c * m + p];
        }
        __syncthreads();
    }
    // L u = b, then L^T w = u: a thread per column of B_b, in place in bw (coalesced across the columns)
    const int j = tid;
    if (j < m) {
        bool finite = true;
        for (int i = 0; i < m; ++i) {
            double s = bw[i * m + j];
            for (int p = 0; p < i; ++p) s -= L[i * m + p] * bw[p * m + j];
            bw[i * m + j] = s / L[i * m + i];
        }
        for (int i = m - 1; i >= 0; --i) {
            double s = bw[i * m + j];
            for (int p = i + 1; p < m; ++p) s -= L[p * m + i] * bw[p * m + j];
            s = s / L[i * m + i];
            bw[i * m + j] = s;
            if (!(fabsf((float)s) < INFINITY)) finite = false;
        }
        if (!finite) *bad = 1;
    }
    __syncthreads();
    const bool failed = *bad != 0;
    if (j < m)
        for (int i = 0; i < m; ++i) Wb[i * m + j] = failed ? 0.f : (float)bw[i * m + j];
    if (tid == 0) status[b] = failed ? 1 : 0;
}

static size_t enkl_weights_lds(int m) { return (size_t)m * m * sizeof(double) + 16; }
static int enkl_weights_threads(int m) { return m <= 32 ? 256 : m <= 64 ? 512 : ENKL_MAX_THREADS; }

extern "C" int sda_enkl_weights(const float* T, int m, int k, const int32_t* offsets, const int32_t* idx, const float* rho, int nblk,
                                float sigma, double* bwork, float* W, int32_t* status, void* stream) {
    int rc = enkl_weights_check(T, m, k, offsets, idx, rho, nblk, sigma, bwork, W, status);
    if (rc != SDA_OK) return rc;
    static bool raised[SDA_MAX_DEVICES];
    rc = sda_raise_dyn_lds((const void*)enkl_weights_kernel, (int)enkl_weights_lds(ENKL_MAX_M), raised);
    if (rc != SDA_OK) return rc;
    hipLaunchKernelGGL(enkl_weights_kernel, dim3((unsigned)nblk), dim3(enkl_weights_threads(m)), enkl_weights_lds(m), (hipStream_t)stream,
                       T, m, k, offsets, idx, rho, sigma, bwork, W, status);
    return sda_launch_status();
}

// ---------------------------------------------------------------- transform: grid (blocks x tiles of a block's components, slabs).
// LDS (dynamic): X[pad16(m)][ENKL_LD] floats, the tile of all members, zero past m and past the block.  The body is
// enkw_transform_kernel's update with the tile's components gathered from the block (rows of bw contiguous floats) and W[b].
__global__ __launch_bounds__(ENKL_THREADS) void enkl_transform_kernel(float* __restrict__ S, int64_t s_st, int64_t s_sp, int m, int C,
                                                                      int Hg, int Wg, int bh, int bw, int ntile,
                                                                      const int32_t* __restrict__ offsets, const float* __restrict__ W) {
    extern __shared__ __attribute__((aligned(16))) char enkl_smem[];
    float* X = (float*)enkl_smem;
    const int tid = threadIdx.x;
    const int b = blockIdx.x / ntile, tile = blockIdx.x % ntile;
    if (offsets[b + 1] <= offsets[b]) return;                // an empty list: nothing of S is read (workgroup-uniform)
    const int mp = enkl_pad16(m), rt = mp >> 4;
    const int nbc = Wg / bw;
    const int br = b / nbc, bc = b % nbc;
    const int64_t nb = (int64_t)C * bh * bw;
    const int64_t q0 = (int64_t)tile * ENKL_TC;
    float* x = S + (int64_t)blockIdx.y * s_st;
    const float* Wb = W + (int64_t)b * m * m;

    {   // the whole tile is read before anything is stored
        const int c = tid & (ENKL_TC - 1);
        const bool c_ok = q0 + c < nb;
        const int64_t off = c_ok ? enkl_offset(q0 + c, br, bc, Hg, Wg, bh, bw) : 0;
        for (int r = tid / ENKL_TC; r < mp; r += ENKL_THREADS / ENKL_TC)
            X[r * ENKL_LD + c] = (r < m && c_ok) ? x[(int64_t)r * s_sp + off] : 0.f;
    }
    __syncthreads();
    if (tid < ENKL_TC) {                                     // column means in float64, in member order; centre in place
        double s = 0.0;
        for (int j = 0; j < m; ++j) s += (double)X[j * ENKL_LD + tid];
        const double mean = s / (double)m;
        for (int j = 0; j < m; ++j) X[j * ENKL_LD + tid] = (float)((double)X[j * ENKL_LD + tid] - mean);
    }
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int ct0 = 2 * wave;
    if (q0 + ct0 * 16 >= nb) return;                         // wave-uniform; no barrier follows
    enkl_f4 acc[ENKL_MAX_M / 16][2];
#pragma unroll
    for (int t = 0; t < ENKL_MAX_M / 16; ++t) acc[t][0] = acc[t][1] = enkl_f4{0.f, 0.f, 0.f, 0.f};
    const int m4 = (m + 3) & ~3;
    for (int m0 = 0; m0 < m4; m0 += 4) {
        const int mm = m0 + kq;                              // < pad16(m): rows m .. are zero
        const float b0 = X[mm * ENKL_LD + ct0 * 16 + r16], b1 = X[mm * ENKL_LD + ct0 * 16 + 16 + r16];
#pragma unroll
        for (int t = 0; t < ENKL_MAX_M / 16; ++t)
            if (t < rt) {                                    // wave-uniform
                const int j = t * 16 + r16;
                const float a = (mm < m && j < m) ? Wb[mm * m + j] : 0.f;
                acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, acc[t][0], 0, 0, 0);
                acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, acc[t][1], 0, 0, 0);
            }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int64_t q = q0 + (ct0 + h) * 16 + r16;
        if (q >= nb) continue;
        const int64_t off = enkl_offset(q, br, bc, Hg, Wg, bh, bw);
#pragma unroll
        for (int t = 0; t < ENKL_MAX_M / 16; ++t)
            if (t < rt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = t * 16 + kq * 4 + r;
                    if (j < m) {
                        float* p = x + (int64_t)j * s_sp + off;
                        *p = *p + (h == 0 ? acc[t][0][r] : acc[t][1][r]);
                    }
                }
            }
    }
}

static size_t enkl_transform_lds(int m) { return (size_t)enkl_pad16(m) * ENKL_LD * sizeof(float); }

extern "C" int sda_enkl_transform(float* S, int64_t s_st, int64_t s_sp, int nslab, int m, int C, int Hg, int Wg, int bh, int bw,
                                  const int32_t* offsets, const float* W, void* stream) {
    int rc = enkl_transform_check(S, s_st, s_sp, nslab, m, C, Hg, Wg, bh, bw, offsets, W);
    if (rc != SDA_OK) return rc;
    static bool raised[SDA_MAX_DEVICES];
    rc = sda_raise_dyn_lds((const void*)enkl_transform_kernel, (int)enkl_transform_lds(ENKL_MAX_M), raised);
    if (rc != SDA_OK) return rc;
    const int nblk = (Hg / bh) * (Wg / bw);
    const int ntile = (int)(((int64_t)C * bh * bw + ENKL_TC - 1) / ENKL_TC);
    hipLaunchKernelGGL(enkl_transform_kernel, dim3((unsigned)(nblk * ntile), (unsigned)nslab), dim3(ENKL_THREADS), enkl_transform_lds(m),
                       (hipStream_t)stream, S, s_st, s_sp, m, C, Hg, Wg, bh, bw, ntile, offsets, W);
    return sda_launch_status();
}

#else  // SDA_HOST_EMU
// ---------------------------------------------------------------- CPU replay (tests only; libsda_emu.so): the same arithmetic in the
// same summation orders.  A matrix instruction is a chain of fused multiply-adds over its 4 values in index order, started from
// its accumulator, so a tile entry is one fma chain over the block's list (the zero padding of the last 4 adds nothing).
#include <vector>

extern "C" int sda_enkl_pack_host(const float* Y, const float* D, int m, int k, float* T) {
    int rc = enkl_pack_check(Y, D, m, k, T);
    if (rc != SDA_OK) return rc;
    for (int i = 0; i < k; ++i)
        for (int r = 0; r < 2 * m; ++r) T[(int64_t)i * 2 * m + r] = r < m ? Y[(int64_t)r * k + i] : D[(int64_t)(r - m) * k + i];
    return SDA_OK;
}

extern "C" int sda_enkl_weights_host(const float* T, int m, int k, const int32_t* offsets, const int32_t* idx, const float* rho, int nblk,
                                     float sigma, double* bwork, float* W, int32_t* status) {
    int rc = enkl_weights_check(T, m, k, offsets, idx, rho, nblk, sigma, bwork, W, status);
    if (rc != SDA_OK) return rc;
    const double s2 = (double)sigma * (double)sigma;
    std::vector<double> L((size_t)m * m);
    for (int b = 0; b < nblk; ++b) {
        const int lo = offsets[b], n = offsets[b + 1] - lo;
        float* Wb = W + (int64_t)b * m * m;
        double* bw = bwork + (int64_t)b * m * m;
        if (n <= 0) {
            for (int e = 0; e < m * m; ++e) Wb[e] = 0.f;
            status[b] = 0;
            continue;
        }
        bool failed = false;
        for (int c = 0; c < n; ++c)
            if ((unsigned)idx[lo + c] >= (unsigned)k) failed = true;
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < m; ++j) {
                double g = 0.0, bb = 0.0;
                for (int c = 0; c < n; ++c) {
                    const int ix = idx[lo + c];
                    if ((unsigned)ix >= (unsigned)k) continue;
                    const float* t = T + (int64_t)ix * 2 * m;
                    const double a = (double)rho[lo + c] * (double)t[i];
                    g = fma(a, (double)t[j], g);
                    bb = fma(a, (double)t[m + j], bb);
                }
                L[i * m + j] = g / (double)(m - 1) + (i == j ? s2 : 0.0);
                bw[i * m + j] = bb / (double)(m - 1);
            }
        for (int p = 0; p < m; ++p) {
            double v = L[p * m + p];
            if (!(v > 0.0) || !(v < INFINITY)) { failed = true; v = 1.0; }
            L[p * m + p] = sqrt(v);
            for (int i = p + 1; i < m; ++i) L[i * m + p] = L[i * m + p] / L[p * m + p];
            for (int i = p + 1; i < m; ++i)
                for (int c = p + 1; c <= i; ++c) L[i * m + c] -= L[i * m + p] * L[c * m + p];
        }
        for (int j = 0; j < m; ++j) {
            for (int i = 0; i < m; ++i) {
                double s = bw[i * m + j];
                for (int p = 0; p < i; ++p) s -= L[i * m + p] * bw[p * m + j];
                bw[i * m + j] = s / L[i * m + i];
            }
            for (int i = m - 1; i >= 0; --i) {
                double s = bw[i * m + j];
                for (int p = i + 1; p < m; ++p) s -= L[p * m + i] * bw[p * m + j];
                s = s / L[i * m + i];
                bw[i * m + j] = s;
                if (!(fabsf((float)s) < INFINITY)) failed = true;
            }
        }
        for (int e = 0; e < m * m; ++e) Wb[e] = failed ? 0.f : (float)bw[e];
        status[b] = failed ? 1 : 0;
    }
    return SDA_OK;
}

extern "C" int sda_enkl_transform_host(float* S, int64_t s_st, int64_t s_sp, int nslab, int m, int C, int Hg, int Wg, int bh, int bw,
                                       const int32_t* offsets, const float* W) {
    int rc = enkl_transform_check(S, s_st, s_sp, nslab, m, C, Hg, Wg, bh, bw, offsets, W);
    if (rc != SDA_OK) return rc;
    const int nbc = Wg / bw, nblk = (Hg / bh) * nbc;
    const int64_t nb = (int64_t)C * bh * bw;
    const int m4 = (m + 3) & ~3;
    std::vector<float> xc(m4, 0.f), out(m);
    for (int b = 0; b < nblk; ++b) {
        if (offsets[b + 1] <= offsets[b]) continue;
        const float* Wb = W + (int64_t)b * m * m;
        const int br = b / nbc, bc = b % nbc;
        for (int sl = 0; sl < nslab; ++sl) {
            float* x = S + (int64_t)sl * s_st;
            for (int64_t q = 0; q < nb; ++q) {
                const int64_t c = enkl_offset(q, br, bc, Hg, Wg, bh, bw);
                double s = 0.0;
                for (int j = 0; j < m; ++j) s += (double)x[(int64_t)j * s_sp + c];
                const double mean = s / (double)m;
                for (int j = 0; j < m; ++j) xc[j] = (float)((double)x[(int64_t)j * s_sp + c] - mean);
                for (int j = 0; j < m; ++j) {
                    float acc = 0.f;
                    for (int mm = 0; mm < m4; ++mm) acc = fmaf(mm < m ? Wb[mm * m + j] : 0.f, xc[mm], acc);
                    out[j] = x[(int64_t)j * s_sp + c] + acc;
                }
                for (int j = 0; j < m; ++j) x[(int64_t)j * s_sp + c] = out[j];
            }
        }
    }
    return SDA_OK;
}
#endif  // SDA_HOST_EMU
