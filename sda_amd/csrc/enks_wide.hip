// Ensemble-space form of the stochastic ensemble Kalman smoother (enks.hip is the observation-space form): for wide states and a
// modest ensemble, M <= 128 members, any number k of observed values, any state width d.  The observed values H = A(members) come
// from the caller, so A is any callable.  Per analysis FOUR launches (plus one for inflation), whatever M, k, d and the window:
//   sda_enkw_prepare    Y = H - hbar, D = (y + sigma eps) - H, eps                  a thread per observed column
//   sda_enkw_gram       per k-chunk the M x 2M float64 partial of [Y Y^T | Y D^T]   v_mfma_f64_16x16x4_f64
//   sda_enkw_solve      partials summed in chunk order, Cholesky, W (fp32), status  one workgroup
//   sda_enkw_transform  x_j += sum_m W[m][j] (x_m - xbar) on every slab and tile    v_mfma_f32_16x16x4_f32
// (include/sda_hip.h states the arithmetic; DESIGN.md section 5.2e-2 the reasons.)  No kernel waits for another workgroup, nothing
// is read back, there are no atomics; every value is written once by the thread that owns it and every sum has a fixed order,
// so results are bitwise reproducible and a slab's result does not depend on the other slabs of the launch.
//
// Under SDA_HOST_EMU the same arithmetic in the same summation orders runs as plain loops over host arrays (bottom of the file).
#include "sda_common.hpp"
#include "philox.hpp"

#include <math.h>

#define ENKW_SALT 0x454E4B53ull     // enks.hip's ENKS_SALT: both smoothers draw the same perturbations
#define ENKW_MAX_M 128              // one M x M float64 table is 128 KiB of the 160 KiB of LDS
#define ENKW_MAX_K (1 << 24)
#define ENKW_KC 512                 // observed values per Gram chunk
#define ENKW_TC 128                 // state components per transform tile
#define ENKW_LD (ENKW_TC + 16)      // LDS row stride of the tile: rows m .. m + 3 of one B operand fall on 64 distinct banks
#define ENKW_THREADS 256
#define ENKW_SOLVE_THREADS 1024
#define ENKW_MAX_SLABS 65535

__host__ __device__ static inline int enkw_pad16(int m) { return (m + 15) & ~15; }
__host__ __device__ static inline int enkw_chunks(int k) { return (k + ENKW_KC - 1) / ENKW_KC; }

static int enkw_shape_check(int m, int k) {
    if (m < 1 || k < 1) return SDA_E_BADARG;
    if (m < 2 || m > ENKW_MAX_M || k > ENKW_MAX_K) return SDA_E_UNSUPPORTED;
    return SDA_OK;
}

static int enkw_prepare_check(const float* H, int m, int k, const float* y, float sigma, int64_t draw, const float* Y, const float* D) {
    if (!H || !y || !Y || !D || draw < 0 || !(sigma > 0.f)) return SDA_E_BADARG;
    return enkw_shape_check(m, k);
}

static int enkw_gram_check(const float* Y, const float* D, int m, int k, const double* part) {
    if (!Y || !D || !part) return SDA_E_BADARG;
    return enkw_shape_check(m, k);
}

static int enkw_solve_check(const double* part, int m, int k, float sigma, const double* bwork, const float* W, const int32_t* status) {
    if (!part || !bwork || !W || !status || !(sigma > 0.f)) return SDA_E_BADARG;
    return enkw_shape_check(m, k);
}

static int enkw_transform_check(const float* S, int64_t s_st, int64_t s_sp, int nslab, int m, int64_t d, const float* W, float inflation,
                                int mode) {
    if (!S || nslab < 1 || m < 1 || d < 1 || s_sp < d || s_st < 0 || (mode != 0 && mode != 1)) return SDA_E_BADARG;
    if (mode == 0 ? !W : !(inflation > 0.f)) return SDA_E_BADARG;
    if (m < 2 || m > ENKW_MAX_M || nslab > ENKW_MAX_SLABS || d > ((int64_t)1 << 37)) return SDA_E_UNSUPPORTED;
    return SDA_OK;
}

extern "C" int64_t sda_enkw_gram_doubles(int m, int k) {
    if (enkw_shape_check(m, k) != SDA_OK) return 0;
    const int64_t mp = enkw_pad16(m);
    return (int64_t)enkw_chunks(k) * mp * 2 * mp;
}

// element c & 3 of quad c >> 2 of row j: eps_j[c] of the salted sda_randn_rows stream
__host__ __device__ __forceinline__ float enkw_noise(uint64_t seed, int j, int64_t draw, int c) {
    const uint64_t s = seed ^ ENKW_SALT;
    float n4[4];
    philox_normal4(c >> 2, (uint64_t)j, draw, (uint32_t)s, (uint32_t)(s >> 32), n4);
    const int i = c & 3;
    return i == 0 ? n4[0] : i == 1 ? n4[1] : i == 2 ? n4[2] : n4[3];
}

#ifndef SDA_HOST_EMU
typedef double enkw_d4 __attribute__((ext_vector_type(4)));
typedef float enkw_f4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- prepare: a thread per observed column, loads coalesced across k
__global__ __launch_bounds__(ENKW_THREADS) void enkw_prepare_kernel(const float* __restrict__ H, int m, int k, const float* __restrict__ y,
                                                                    float sigma, uint64_t seed, int64_t draw, float* __restrict__ Y,
                                                                    float* __restrict__ D, float* __restrict__ eps) {
    const int c = blockIdx.x * ENKW_THREADS + threadIdx.x;
    if (c >= k) return;
    double s = 0.0;
    for (int j = 0; j < m; ++j) s += (double)H[(int64_t)j * k + c];
    const double hbar = s / (double)m;
    const float yc = y[c];
    for (int j = 0; j < m; ++j) {
        const int64_t e = (int64_t)j * k + c;
        const float h = H[e];
        const float n = enkw_noise(seed, j, draw, c);
        Y[e] = (float)((double)h - hbar);
        D[e] = (yc + sigma * n) - h;
        if (eps) eps[e] = n;
    }
}

extern "C" int sda_enkw_prepare(const float* H, int m, int k, const float* y, float sigma, uint64_t seed, int64_t draw, float* Y, float* D,
                                float* eps, void* stream) {
    int rc = enkw_prepare_check(H, m, k, y, sigma, draw, Y, D);
    if (rc != SDA_OK) return rc;
    hipLaunchKernelGGL(enkw_prepare_kernel, dim3((unsigned)((k + ENKW_THREADS - 1) / ENKW_THREADS)), dim3(ENKW_THREADS), 0,
                       (hipStream_t)stream, H, m, k, y, sigma, seed, draw, Y, D, eps);
    return sda_launch_status();
}

// ---------------------------------------------------------------- Gram: grid (k-chunks, 16-row tiles); wave w of the 4 owns the
// 16-column tiles w, w + 4, .. of [Y Y^T | Y D^T].  One float64 MFMA covers 4 observed values: lane l holds row (l & 15) of its tile
// at value (l >> 4), for both operands (an NT product), and the accumulator chains the chunk's values in index order.  Rows past M
// and values past k enter as zeros.
__global__ __launch_bounds__(ENKW_THREADS) void enkw_gram_kernel(const float* __restrict__ Y, const float* __restrict__ D, int m, int k,
                                                                 double* __restrict__ part) {
    const int mp = enkw_pad16(m), rt = mp >> 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int c_lo = blockIdx.x * ENKW_KC;
    const int c_hi = min(k, c_lo + ENKW_KC);
    const int row = blockIdx.y * 16 + r16;
    const float* arow = Y + (int64_t)row * k;
    const bool a_ok = row < m;
    const float* brow[4];
    bool b_ok[4], live[4];
    enkw_d4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ct = wave + 4 * i;
        live[i] = ct < 2 * rt;
        const int col = (ct < rt ? ct : ct - rt) * 16 + r16;
        b_ok[i] = live[i] && col < m;
        brow[i] = (ct < rt ? Y : D) + (int64_t)(b_ok[i] ? col : 0) * k;
        acc[i] = enkw_d4{0.0, 0.0, 0.0, 0.0};
    }
    for (int c0 = c_lo; c0 < c_hi; c0 += 4) {
        const int c = c0 + kq;
        const bool in = c < c_hi;
        const double a = (a_ok && in) ? (double)arow[c] : 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (live[i]) {                                   // wave-uniform
                const double b = (b_ok[i] && in) ? (double)brow[i][c] : 0.0;
                acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
            }
    }
    double* out = part + (int64_t)blockIdx.x * mp * 2 * mp;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (live[i]) {
            const int col = (wave + 4 * i) * 16 + r16;
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(int64_t)(blockIdx.y * 16 + kq + 4 * r) * 2 * mp + col] = acc[i][r];
        }
}

extern "C" int sda_enkw_gram(const float* Y, const float* D, int m, int k, double* part, void* stream) {
    int rc = enkw_gram_check(Y, D, m, k, part);
    if (rc != SDA_OK) return rc;
    hipLaunchKernelGGL(enkw_gram_kernel, dim3((unsigned)enkw_chunks(k), (unsigned)(enkw_pad16(m) >> 4)), dim3(ENKW_THREADS), 0,
                       (hipStream_t)stream, Y, D, m, k, part);
    return sda_launch_status();
}

// ---------------------------------------------------------------- solve: ONE workgroup.  LDS (dynamic): L[m][m] doubles, one flag.
__global__ __launch_bounds__(ENKW_SOLVE_THREADS) void enkw_solve_kernel(const double* __restrict__ part, int m, int k, float sigma,
                                                                        double* __restrict__ bw, float* __restrict__ W,
                                                                        int32_t* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char enkw_smem[];
    double* L = (double*)enkw_smem;
    int* bad = (int*)(L + m * m);
    const int tid = threadIdx.x;
    const int mp = enkw_pad16(m), nch = enkw_chunks(k);
    const double s2 = (double)sigma * (double)sigma;
    if (tid == 0) *bad = 0;
    for (int e = tid; e < m * m; e += ENKW_SOLVE_THREADS) {
        const int i = e / m, j = e % m;
        double g = 0.0, b = 0.0;
        for (int ch = 0; ch < nch; ++ch) {
            const double* p = part + ((int64_t)ch * mp + i) * 2 * mp;
            g += p[j];
            b += p[mp + j];
        }
        L[e] = g / (double)(m - 1) + (i == j ? s2 : 0.0);
        bw[e] = b / (double)(m - 1);
    }
    __syncthreads();
    // Cholesky, right-looking, in the lower triangle of L
    for (int p = 0; p < m; ++p) {
        if (tid == 0) {
            double v = L[p * m + p];
            if (!(v > 0.0) || !(v < INFINITY)) { *bad = 1; v = 1.0; }
            L[p * m + p] = sqrt(v);
        }
        __syncthreads();
        const double piv = L[p * m + p];
        for (int i = p + 1 + tid; i < m; i += ENKW_SOLVE_THREADS) L[i * m + p] = L[i * m + p] / piv;
        __syncthreads();
        const int n = m - p - 1;
        for (int e = tid; e < n * n; e += ENKW_SOLVE_THREADS) {
            const int i = p + 1 + e / n, c = p + 1 + e % n;
            if (c <= i) L[i * m + c] -= L[i * m + p] * L[c * m + p];
        }
        __syncthreads();
    }
    // L u = b, then L^T w = u: a thread per column of B, in place in bw (coalesced across the columns)
    const int j = tid;
    bool finite = true;
    if (j < m) {
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
            const float w = (float)s;
            if (!(fabsf(w) < INFINITY)) finite = false;
        }
        if (!finite) *bad = 1;                               // every writer stores the same value
    }
    __syncthreads();
    const bool failed = *bad != 0;
    if (j < m)
        for (int i = 0; i < m; ++i) W[i * m + j] = failed ? 0.f : (float)bw[i * m + j];
    if (tid == 0) status[0] = failed ? 1 : 0;
}

static size_t enkw_solve_lds(int m) { return (size_t)m * m * sizeof(double) + 16; }

extern "C" int sda_enkw_solve(const double* part, int m, int k, float sigma, double* bwork, float* W, int32_t* status, void* stream) {
    int rc = enkw_solve_check(part, m, k, sigma, bwork, W, status);
    if (rc != SDA_OK) return rc;
    static bool raised[SDA_MAX_DEVICES];
    rc = sda_raise_dyn_lds((const void*)enkw_solve_kernel, (int)enkw_solve_lds(ENKW_MAX_M), raised);
    if (rc != SDA_OK) return rc;
    hipLaunchKernelGGL(enkw_solve_kernel, dim3(1), dim3(ENKW_SOLVE_THREADS), enkw_solve_lds(m), (hipStream_t)stream, part, m, k, sigma,
                       bwork, W, status);
    return sda_launch_status();
}

// ---------------------------------------------------------------- transform: grid (tiles of d, slabs).  LDS (dynamic):
// X[pad16(m)][ENKW_LD] floats, the tile of all members, zero past m and past d.  mode 0: the update; mode 1: inflation.
// Wave w of the 4 owns the 16-component tiles 2w and 2w + 1 for every 16-member tile of the output: out[j][c] = sum_m W[m][j] Xc[m][c],
// A operand W^T (lane l: member j = l & 15 of the tile, summed member l >> 4), B operand the centred tile.
__global__ __launch_bounds__(ENKW_THREADS) void enkw_transform_kernel(float* __restrict__ S, int64_t s_st, int64_t s_sp, int m, int64_t d,
                                                                      const float* __restrict__ W, float lam, int mode) {
    extern __shared__ __attribute__((aligned(16))) char enkw_smem[];
    float* X = (float*)enkw_smem;
    const int tid = threadIdx.x;
    const int mp = enkw_pad16(m), rt = mp >> 4;
    const int64_t c0 = (int64_t)blockIdx.x * ENKW_TC;
    float* x = S + (int64_t)blockIdx.y * s_st;

    {   // the whole tile is read before anything is stored
        const int c = tid & (ENKW_TC - 1);
        const bool c_ok = c0 + c < d;
        for (int r = tid / ENKW_TC; r < mp; r += ENKW_THREADS / ENKW_TC)
            X[r * ENKW_LD + c] = (r < m && c_ok) ? x[(int64_t)r * s_sp + c0 + c] : 0.f;
    }
    __syncthreads();
    if (tid < ENKW_TC) {                                     // column means in float64, in member order; centre in place
        double s = 0.0;
        for (int j = 0; j < m; ++j) s += (double)X[j * ENKW_LD + tid];
        const double mean = s / (double)m;
        if (mode == 1) {
            const float mu = (float)mean, lm1 = lam - 1.0f;
            if (c0 + tid < d)
                for (int j = 0; j < m; ++j) {
                    const float v = X[j * ENKW_LD + tid];
                    x[(int64_t)j * s_sp + c0 + tid] = v + lm1 * (v - mu);
                }
        } else {
            for (int j = 0; j < m; ++j) X[j * ENKW_LD + tid] = (float)((double)X[j * ENKW_LD + tid] - mean);
        }
    }
    if (mode == 1) return;
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int ct0 = 2 * wave;
    if (c0 + ct0 * 16 >= d) return;                          // wave-uniform; no barrier follows
    enkw_f4 acc[ENKW_MAX_M / 16][2];
#pragma unroll
    for (int t = 0; t < ENKW_MAX_M / 16; ++t) acc[t][0] = acc[t][1] = enkw_f4{0.f, 0.f, 0.f, 0.f};
    const int m4 = (m + 3) & ~3;
    for (int m0 = 0; m0 < m4; m0 += 4) {
        const int mm = m0 + kq;                              // < pad16(m): rows m .. are zero
        const float b0 = X[mm * ENKW_LD + ct0 * 16 + r16], b1 = X[mm * ENKW_LD + ct0 * 16 + 16 + r16];
#pragma unroll
        for (int t = 0; t < ENKW_MAX_M / 16; ++t)
            if (t < rt) {                                    // wave-uniform
                const int j = t * 16 + r16;
                const float a = (mm < m && j < m) ? W[mm * m + j] : 0.f;
                acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, acc[t][0], 0, 0, 0);
                acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, acc[t][1], 0, 0, 0);
            }
    }
#pragma unroll
    for (int t = 0; t < ENKW_MAX_M / 16; ++t)
        if (t < rt) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int64_t c = c0 + (ct0 + h) * 16 + r16;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = t * 16 + kq * 4 + r;
                    if (j < m && c < d) {
                        float* p = x + (int64_t)j * s_sp + c;
                        *p = *p + acc[t][h][r];
                    }
                }
            }
        }
}

static size_t enkw_transform_lds(int m) { return (size_t)enkw_pad16(m) * ENKW_LD * sizeof(float); }

extern "C" int sda_enkw_transform(float* S, int64_t s_st, int64_t s_sp, int nslab, int m, int64_t d, const float* W, float inflation,
                                  int mode, void* stream) {
    int rc = enkw_transform_check(S, s_st, s_sp, nslab, m, d, W, inflation, mode);
    if (rc != SDA_OK) return rc;
    if (mode == 1 && inflation == 1.0f) return SDA_OK;       // lambda == 1 touches nothing
    static bool raised[SDA_MAX_DEVICES];
    rc = sda_raise_dyn_lds((const void*)enkw_transform_kernel, (int)enkw_transform_lds(ENKW_MAX_M), raised);
    if (rc != SDA_OK) return rc;
    hipLaunchKernelGGL(enkw_transform_kernel, dim3((unsigned)((d + ENKW_TC - 1) / ENKW_TC), (unsigned)nslab), dim3(ENKW_THREADS),
                       enkw_transform_lds(m), (hipStream_t)stream, S, s_st, s_sp, m, d, W, inflation, mode);
    return sda_launch_status();
}

#else  // SDA_HOST_EMU
// ---------------------------------------------------------------- CPU replay (tests only; libsda_emu.so): the same arithmetic in the
// same summation orders.  A matrix instruction is a chain of fused multiply-adds over its 4 values in index order, started from
// its accumulator, so a chunk (a tile column) is one fma chain over its zero-padded length.
#include <vector>

// eps_in (may be null): perturbations to use instead of the generator's, so a caller can replay another run's draws exactly
extern "C" int sda_enkw_prepare_host(const float* H, int m, int k, const float* y, float sigma, uint64_t seed, int64_t draw, float* Y,
                                     float* D, float* eps, const float* eps_in) {
    int rc = enkw_prepare_check(H, m, k, y, sigma, draw, Y, D);
    if (rc != SDA_OK) return rc;
    for (int c = 0; c < k; ++c) {
        double s = 0.0;
        for (int j = 0; j < m; ++j) s += (double)H[(int64_t)j * k + c];
        const double hbar = s / (double)m;
        for (int j = 0; j < m; ++j) {
            const int64_t e = (int64_t)j * k + c;
            const float h = H[e];
            const float n = eps_in ? eps_in[e] : enkw_noise(seed, j, draw, c);
            Y[e] = (float)((double)h - hbar);
            D[e] = (y[c] + sigma * n) - h;
            if (eps) eps[e] = n;
        }
    }
    return SDA_OK;
}

extern "C" int sda_enkw_gram_host(const float* Y, const float* D, int m, int k, double* part) {
    int rc = enkw_gram_check(Y, D, m, k, part);
    if (rc != SDA_OK) return rc;
    const int mp = enkw_pad16(m), nch = enkw_chunks(k);
    for (int ch = 0; ch < nch; ++ch) {
        const int c_lo = ch * ENKW_KC, c_hi = k < c_lo + ENKW_KC ? k : c_lo + ENKW_KC;
        for (int i = 0; i < mp; ++i)
            for (int jj = 0; jj < 2 * mp; ++jj) {
                const int j = jj < mp ? jj : jj - mp;
                const float* src = jj < mp ? Y : D;
                double acc = 0.0;
                if (i < m && j < m)
                    for (int c = c_lo; c < c_hi; ++c) acc = fma((double)Y[(int64_t)i * k + c], (double)src[(int64_t)j * k + c], acc);
                part[((int64_t)ch * mp + i) * 2 * mp + jj] = acc;
            }
    }
    return SDA_OK;
}

extern "C" int sda_enkw_solve_host(const double* part, int m, int k, float sigma, double* bw, float* W, int32_t* status) {
    int rc = enkw_solve_check(part, m, k, sigma, bw, W, status);
    if (rc != SDA_OK) return rc;
    const int mp = enkw_pad16(m), nch = enkw_chunks(k);
    const double s2 = (double)sigma * (double)sigma;
    std::vector<double> L((size_t)m * m);
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) {
            double g = 0.0, b = 0.0;
            for (int ch = 0; ch < nch; ++ch) {
                const double* p = part + ((int64_t)ch * mp + i) * 2 * mp;
                g += p[j];
                b += p[mp + j];
            }
            L[i * m + j] = g / (double)(m - 1) + (i == j ? s2 : 0.0);
            bw[i * m + j] = b / (double)(m - 1);
        }
    bool failed = false;
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
    for (int e = 0; e < m * m; ++e) W[e] = failed ? 0.f : (float)bw[e];
    status[0] = failed ? 1 : 0;
    return SDA_OK;
}

extern "C" int sda_enkw_transform_host(float* S, int64_t s_st, int64_t s_sp, int nslab, int m, int64_t d, const float* W, float inflation,
                                       int mode) {
    int rc = enkw_transform_check(S, s_st, s_sp, nslab, m, d, W, inflation, mode);
    if (rc != SDA_OK) return rc;
    if (mode == 1 && inflation == 1.0f) return SDA_OK;
    const int m4 = (m + 3) & ~3;
    std::vector<float> xc(m4, 0.f), out(m);
    for (int sl = 0; sl < nslab; ++sl) {
        float* x = S + (int64_t)sl * s_st;
        for (int64_t c = 0; c < d; ++c) {
            double s = 0.0;
            for (int j = 0; j < m; ++j) s += (double)x[(int64_t)j * s_sp + c];
            const double mean = s / (double)m;
            if (mode == 1) {
                const float mu = (float)mean, lm1 = inflation - 1.0f;
                for (int j = 0; j < m; ++j) {
                    const float v = x[(int64_t)j * s_sp + c];
                    x[(int64_t)j * s_sp + c] = v + lm1 * (v - mu);
                }
                continue;
            }
            for (int j = 0; j < m; ++j) xc[j] = (float)((double)x[(int64_t)j * s_sp + c] - mean);
            for (int j = 0; j < m; ++j) {
                float acc = 0.f;
                for (int mm = 0; mm < m4; ++mm) acc = fmaf(mm < m ? W[mm * m + j] : 0.f, xc[mm], acc);
                out[j] = x[(int64_t)j * s_sp + c] + acc;
            }
            for (int j = 0; j < m; ++j) x[(int64_t)j * s_sp + c] = out[j];
        }
    }
    return SDA_OK;
}
#endif  // SDA_HOST_EMU
