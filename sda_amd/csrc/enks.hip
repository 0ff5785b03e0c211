// Stochastic (perturbed-observation) ensemble Kalman smoother, the third Lorenz baseline beside the particle filter and 4D-Var:
// per observation ONE launch for the gain (sda_enks_gain: observed anomalies, innovation covariance, its Cholesky factor and the
// perturbed innovations solved against it) and ONE for the update of every slab of the smoothing window (sda_enks_update), whatever
// the ensemble size, the number of observed components or the window length.  No kernel waits for another workgroup, nothing is
// read back, there are no atomics: every value is written once by the thread that owns it, every reduction over the members has
// an order fixed by the member count alone, so results are bitwise reproducible and a slab's result does not depend on the grid.
//
// Numerics: the ensemble is fp32; every sum over the members, the k x k covariance, its factor, its inverse and the two skinny
// products accumulate in float64 on the vector ALU.  The fp32 matrix cores are NOT used: an fp32 MFMA is an fp32 fma chain, and an
// fp32 chain over thousands of members misses the project's error rule (3 x the error of an fp32 replay that sums pairwise), while
// the float64 operands here are few.
//
// Under SDA_HOST_EMU the same arithmetic runs as plain loops over host arrays (bottom of the file; libsda_emu.so).
#include "sda_common.hpp"
#include "chain_check.hpp"
#include "philox.hpp"

#define ENKS_SALT 0x454E4B53ull     // 'ENKS': keeps the perturbations off the chain's own transition noise under the same seed
#define ENKS_MAX_M (1 << 22)
#define ENKS_MAX_D 64
#define ENKS_GAIN_THREADS 1024
#define ENKS_UPD_THREADS 512
#define ENKS_RB 8                   // rows of a / z a thread carries at a time

// the observed value of one state component (the affine selection of sda_chain_obs), after inflation about the member mean
__host__ __device__ __forceinline__ float enks_inflate(float x, float mean, float lam) { return mean + lam * (x - mean); }
__host__ __device__ __forceinline__ float enks_observe(float x, float shift, float scale) { return (x - shift) / scale; }

// elements 4q .. 4q+3 of row j in draw `draw` of the sda_randn_rows stream under the salted seed
__host__ __device__ __forceinline__ void enks_noise4(uint64_t seed, uint64_t j, int64_t draw, int64_t q, float* e) {
    const uint64_t s = seed ^ ENKS_SALT;
    philox_normal4(q, j, draw, (uint32_t)s, (uint32_t)(s >> 32), e);
}

static int enks_gain_check(const float* x, int m, int64_t sp, int d, const sda_chain_obs* obs, float inflation, int64_t draw,
                           const float* a, const float* z, const float* work, const int32_t* status) {
    if (!x || !a || !z || !work || !status || m < 2 || d < 1 || sp < d || draw < 0 || !(inflation > 0.f)) return SDA_E_BADARG;
    if (d > ENKS_MAX_D || m > ENKS_MAX_M) return SDA_E_UNSUPPORTED;
    return chain_obs_check(obs, d);
}

static int enks_update_check(const float* S, int64_t s_st, int64_t s_sp, int nslab, int m, int d, int k, float inflation,
                             const float* a, const float* z) {
    if (!S || !a || !z || nslab < 1 || m < 2 || d < 1 || k < 1 || k > d || s_sp < d || s_st < 0 || !(inflation > 0.f))
        return SDA_E_BADARG;
    if (d > ENKS_MAX_D || k > SDA_CHAIN_MAXOBS || m > ENKS_MAX_M || nslab > 0x7fffffff / 2) return SDA_E_UNSUPPORTED;
    return SDA_OK;
}

#ifndef SDA_HOST_EMU
// ---------------------------------------------------------------- device kernels
// ONE workgroup.  LDS (dynamic): C[k][k], L[k][k] doubles, xm[k], hb[k] doubles, one flag.
__global__ __launch_bounds__(ENKS_GAIN_THREADS) void enks_gain_kernel(const float* __restrict__ x, int m, int64_t sp, sda_chain_obs obs,
                                                                      float lam, uint64_t seed, int64_t draw, float* __restrict__ a,
                                                                      float* __restrict__ z, float* __restrict__ work,
                                                                      int32_t* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char enks_smem[];
    const int k = obs.k;
    double* C = (double*)enks_smem;
    double* L = C + k * k;
    double* xm = L + k * k;
    double* hb = xm + SDA_CHAIN_MAXOBS;
    int* bad = (int*)(hb + SDA_CHAIN_MAXOBS);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int NW = ENKS_GAIN_THREADS / SDA_WAVE;
    if (tid == 0) *bad = 0;

    // step 2: h = obs(inflated x), h-bar, a = h - h-bar.  One wave per observed row, lanes over the members.
    for (int r = wave; r < k; r += NW) {
        const int c = obs.idx[r];
        float mean = 0.f;
        if (lam != 1.0f) {
            double s = 0.0;
            for (int j = lane; j < m; j += SDA_WAVE) s += (double)x[(int64_t)j * sp + c];
            s = sda_wave_sum(s);
            mean = (float)(__shfl(s, 0, SDA_WAVE) / (double)m);
        }
        double s = 0.0;
        for (int j = lane; j < m; j += SDA_WAVE) {
            float v = x[(int64_t)j * sp + c];
            if (lam != 1.0f) v = enks_inflate(v, mean, lam);
            const float h = enks_observe(v, obs.shift[r], obs.scale[r]);
            work[(int64_t)r * m + j] = h;
            s += (double)h;
        }
        s = sda_wave_sum(s);
        const double hbar = __shfl(s, 0, SDA_WAVE) / (double)m;
        for (int j = lane; j < m; j += SDA_WAVE) a[(int64_t)r * m + j] = (float)((double)work[(int64_t)r * m + j] - hbar);
    }
    __syncthreads();

    // step 3: C = a a^T / (M - 1) + sigma^2 I, one wave per entry of the lower triangle
    const double s2 = (double)obs.sigma * (double)obs.sigma;
    for (int r = 0, p = 0; r < k; ++r)
        for (int c = 0; c <= r; ++c, ++p) {
            if (p % NW != wave) continue;
            double s = 0.0;
            for (int j = lane; j < m; j += SDA_WAVE) s += (double)a[(int64_t)r * m + j] * (double)a[(int64_t)c * m + j];
            s = sda_wave_sum(s);
            if (lane == 0) {
                const double v = s / (double)(m - 1) + (r == c ? s2 : 0.0);
                C[r * k + c] = v;
                C[c * k + r] = v;
            }
        }
    __syncthreads();

    // Cholesky, right-looking, in the lower triangle of C
    for (int p = 0; p < k; ++p) {
        if (tid == 0) {
            double v = C[p * k + p];
            if (!(v > 0.0) || !(v < INFINITY)) { *bad = 1; v = 1.0; }
            C[p * k + p] = sqrt(v);
        }
        __syncthreads();
        const double piv = C[p * k + p];
        for (int i = p + 1 + tid; i < k; i += ENKS_GAIN_THREADS) C[i * k + p] = C[i * k + p] / piv;
        __syncthreads();
        const int n = k - p - 1;
        for (int e = tid; e < n * n; e += ENKS_GAIN_THREADS) {
            const int i = p + 1 + e / n, c = p + 1 + e % n;
            if (c <= i) C[i * k + c] -= C[i * k + p] * C[c * k + p];
        }
        __syncthreads();
    }
    // L^-1 by columns (forward substitution), then C^-1 = L^-T L^-1 over C
    for (int c = tid; c < k; c += ENKS_GAIN_THREADS) {
        for (int i = 0; i < c; ++i) L[i * k + c] = 0.0;
        L[c * k + c] = 1.0 / C[c * k + c];
        for (int i = c + 1; i < k; ++i) {
            double s = 0.0;
            for (int p = c; p < i; ++p) s += C[i * k + p] * L[p * k + c];
            L[i * k + c] = -s / C[i * k + i];
        }
    }
    __syncthreads();
    for (int e = tid; e < k * k; e += ENKS_GAIN_THREADS) {
        const int r = e / k, c = e % k;
        double s = 0.0;
        for (int p = (r > c ? r : c); p < k; ++p) s += L[p * k + r] * L[p * k + c];
        C[e] = s;
    }
    // step 4: the perturbed innovation (y + sigma eps) - h over work, then z = C^-1 innovation
    const int quads = (k + 3) / 4;
    for (int64_t e = tid; e < (int64_t)m * quads; e += ENKS_GAIN_THREADS) {
        const int j = (int)(e % m), q = (int)(e / m);
        float n4[4];
        enks_noise4(seed, (uint64_t)j, draw, q, n4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 4 * q + i;
            if (r < k) work[(int64_t)r * m + j] = (obs.y[r] + obs.sigma * n4[i]) - work[(int64_t)r * m + j];
        }
    }
    __syncthreads();
    const bool failed = *bad != 0;
    for (int j = tid; j < m; j += ENKS_GAIN_THREADS) {
        for (int rb = 0; rb < k; rb += ENKS_RB) {
            double acc[ENKS_RB];
#pragma unroll
            for (int i = 0; i < ENKS_RB; ++i) acc[i] = 0.0;
            for (int c = 0; c < k; ++c) {
                const double v = (double)work[(int64_t)c * m + j];
#pragma unroll
                for (int i = 0; i < ENKS_RB; ++i)
                    if (rb + i < k) acc[i] += C[(rb + i) * k + c] * v;
            }
#pragma unroll
            for (int i = 0; i < ENKS_RB; ++i)
                if (rb + i < k) z[(int64_t)(rb + i) * m + j] = failed ? 0.f : (float)acc[i];
        }
    }
    if (tid == 0) status[0] = failed ? 1 : 0;
}

static size_t enks_gain_lds(int k) { return (size_t)(2 * k * k + 2 * SDA_CHAIN_MAXOBS) * sizeof(double) + 16; }

extern "C" int sda_enks_gain(const float* x, int m, int64_t sp, int d, const sda_chain_obs* obs, float inflation, uint64_t seed,
                             int64_t draw, float* a, float* z, float* work, int32_t* status, void* stream) {
    int rc = enks_gain_check(x, m, sp, d, obs, inflation, draw, a, z, work, status);
    if (rc != SDA_OK) return rc;
    static bool raised[SDA_MAX_DEVICES];
    rc = sda_raise_dyn_lds((const void*)enks_gain_kernel, (int)enks_gain_lds(SDA_CHAIN_MAXOBS), raised);
    if (rc != SDA_OK) return rc;
    hipLaunchKernelGGL(enks_gain_kernel, dim3(1), dim3(ENKS_GAIN_THREADS), enks_gain_lds(obs->k), (hipStream_t)stream, x, m, sp, *obs,
                       inflation, seed, draw, a, z, work, status);
    return sda_launch_status();
}

// One workgroup per slab of the window.  A pass covers G = THREADS / d members as G d consecutive floats (particle stride == d):
// thread tid holds component tid % d of member pass G + tid / d, so a wave's loads are contiguous for d = 3 as for d = 40.
// LDS (dynamic): part[THREADS][RB] doubles, p[d][k] doubles, xbar[d] doubles.
__global__ __launch_bounds__(ENKS_UPD_THREADS) void enks_update_kernel(float* __restrict__ S, int64_t s_st, int64_t s_sp, int nslab, int m,
                                                                       int d, int k, float lam, const float* __restrict__ a,
                                                                       const float* __restrict__ z) {
    extern __shared__ __attribute__((aligned(16))) char enks_smem[];
    double* part = (double*)enks_smem;
    double* P = part + ENKS_UPD_THREADS * ENKS_RB;
    double* xbar = P + d * k;
    const int tid = threadIdx.x;
    const int G = ENKS_UPD_THREADS / d;
    const bool live = tid < G * d;
    const int c = tid % d, g = tid / d;
    const int passes = (m + G - 1) / G;
    float* x = S + (int64_t)blockIdx.x * s_st;

    // the member mean of every component: per-thread sums in member order, then one ordered combine
    double s = 0.0;
    if (live)
        for (int ps = 0; ps < passes; ++ps) {
            const int j = ps * G + g;
            if (j < m) s += (double)x[(int64_t)j * s_sp + c];
        }
    part[tid] = s;
    __syncthreads();
    if (tid < d) {
        double t = 0.0;
        for (int q = 0; q < G; ++q) t += part[q * d + tid];
        xbar[tid] = t / (double)m;
    }
    __syncthreads();
    // step 1: inflation, on the last slab of the window only; lambda == 1 leaves it untouched bit for bit
    if (lam != 1.0f && (int)blockIdx.x == nslab - 1) {
        if (live) {
            const float mean = (float)xbar[c];
            for (int ps = 0; ps < passes; ++ps) {
                const int j = ps * G + g;
                if (j < m) x[(int64_t)j * s_sp + c] = enks_inflate(x[(int64_t)j * s_sp + c], mean, lam);
            }
        }
        __syncthreads();
    }
    // step 5a: p[c][r] = sum_j (x_j[c] - xbar[c]) a_j[r] / (M - 1), ENKS_RB rows at a time
    const double mean = live ? xbar[c] : 0.0;
    for (int rb = 0; rb < k; rb += ENKS_RB) {
        double acc[ENKS_RB];
#pragma unroll
        for (int i = 0; i < ENKS_RB; ++i) acc[i] = 0.0;
        if (live)
            for (int ps = 0; ps < passes; ++ps) {
                const int j = ps * G + g;
                if (j < m) {
                    const double dx = (double)x[(int64_t)j * s_sp + c] - mean;
#pragma unroll
                    for (int i = 0; i < ENKS_RB; ++i)
                        if (rb + i < k) acc[i] += dx * (double)a[(int64_t)(rb + i) * m + j];
                }
            }
#pragma unroll
        for (int i = 0; i < ENKS_RB; ++i) part[tid * ENKS_RB + i] = acc[i];
        __syncthreads();
        for (int e = tid; e < d * ENKS_RB; e += ENKS_UPD_THREADS) {
            const int cc = e / ENKS_RB, i = e % ENKS_RB;
            if (rb + i < k) {
                double t = 0.0;
                for (int q = 0; q < G; ++q) t += part[(q * d + cc) * ENKS_RB + i];
                P[cc * k + rb + i] = t / (double)(m - 1);
            }
        }
        __syncthreads();
    }
    // step 5b: x_j[c] += p[c] . z_j
    if (live)
        for (int ps = 0; ps < passes; ++ps) {
            const int j = ps * G + g;
            if (j < m) {
                double inc = 0.0;
                for (int r = 0; r < k; ++r) inc += P[c * k + r] * (double)z[(int64_t)r * m + j];
                float* px = x + (int64_t)j * s_sp + c;
                *px = (float)((double)*px + inc);
            }
        }
}

static size_t enks_update_lds(int d, int k) { return (size_t)(ENKS_UPD_THREADS * ENKS_RB + d * k + d) * sizeof(double); }

extern "C" int sda_enks_update(float* S, int64_t s_st, int64_t s_sp, int nslab, int m, int d, int k, float inflation, const float* a,
                               const float* z, void* stream) {
    int rc = enks_update_check(S, s_st, s_sp, nslab, m, d, k, inflation, a, z);
    if (rc != SDA_OK) return rc;
    static bool raised[SDA_MAX_DEVICES];
    rc = sda_raise_dyn_lds((const void*)enks_update_kernel, (int)enks_update_lds(ENKS_MAX_D, SDA_CHAIN_MAXOBS), raised);
    if (rc != SDA_OK) return rc;
    hipLaunchKernelGGL(enks_update_kernel, dim3((unsigned)nslab), dim3(ENKS_UPD_THREADS), enks_update_lds(d, k), (hipStream_t)stream, S,
                       s_st, s_sp, nslab, m, d, k, inflation, a, z);
    return sda_launch_status();
}

#else  // SDA_HOST_EMU
// ---------------------------------------------------------------- CPU replay (tests only; libsda_emu.so): the same arithmetic as
// plain loops over HOST arrays.  Sums over the members run in index order where the device combines per-lane partial sums.
#include <vector>

extern "C" int sda_enks_gain_host(const float* x, int m, int64_t sp, int d, const sda_chain_obs* obs, float inflation, uint64_t seed,
                                  int64_t draw, float* a, float* z, float* work, int32_t* status) {
    int rc = enks_gain_check(x, m, sp, d, obs, inflation, draw, a, z, work, status);
    if (rc != SDA_OK) return rc;
    const int k = obs->k;
    const float lam = inflation;
    for (int r = 0; r < k; ++r) {
        const int c = obs->idx[r];
        float mean = 0.f;
        if (lam != 1.0f) {
            double s = 0.0;
            for (int j = 0; j < m; ++j) s += (double)x[(int64_t)j * sp + c];
            mean = (float)(s / (double)m);
        }
        double s = 0.0;
        for (int j = 0; j < m; ++j) {
            float v = x[(int64_t)j * sp + c];
            if (lam != 1.0f) v = enks_inflate(v, mean, lam);
            const float h = enks_observe(v, obs->shift[r], obs->scale[r]);
            work[(int64_t)r * m + j] = h;
            s += (double)h;
        }
        const double hbar = s / (double)m;
        for (int j = 0; j < m; ++j) a[(int64_t)r * m + j] = (float)((double)work[(int64_t)r * m + j] - hbar);
    }
    std::vector<double> C((size_t)k * k), L((size_t)k * k, 0.0);
    const double s2 = (double)obs->sigma * (double)obs->sigma;
    for (int r = 0; r < k; ++r)
        for (int c = 0; c <= r; ++c) {
            double s = 0.0;
            for (int j = 0; j < m; ++j) s += (double)a[(int64_t)r * m + j] * (double)a[(int64_t)c * m + j];
            C[r * k + c] = C[c * k + r] = s / (double)(m - 1) + (r == c ? s2 : 0.0);
        }
    bool failed = false;
    for (int p = 0; p < k; ++p) {
        double v = C[p * k + p];
        if (!(v > 0.0) || !(v < INFINITY)) { failed = true; v = 1.0; }
        C[p * k + p] = sqrt(v);
        for (int i = p + 1; i < k; ++i) C[i * k + p] = C[i * k + p] / C[p * k + p];
        for (int i = p + 1; i < k; ++i)
            for (int c = p + 1; c <= i; ++c) C[i * k + c] -= C[i * k + p] * C[c * k + p];
    }
    for (int c = 0; c < k; ++c) {
        L[c * k + c] = 1.0 / C[c * k + c];
        for (int i = c + 1; i < k; ++i) {
            double s = 0.0;
            for (int p = c; p < i; ++p) s += C[i * k + p] * L[p * k + c];
            L[i * k + c] = -s / C[i * k + i];
        }
    }
    for (int r = 0; r < k; ++r)
        for (int c = 0; c < k; ++c) {
            double s = 0.0;
            for (int p = (r > c ? r : c); p < k; ++p) s += L[p * k + r] * L[p * k + c];
            C[r * k + c] = s;
        }
    for (int j = 0; j < m; ++j)
        for (int q = 0; 4 * q < k; ++q) {
            float n4[4];
            enks_noise4(seed, (uint64_t)j, draw, q, n4);
            for (int i = 0; i < 4 && 4 * q + i < k; ++i) {
                const int r = 4 * q + i;
                work[(int64_t)r * m + j] = (obs->y[r] + obs->sigma * n4[i]) - work[(int64_t)r * m + j];
            }
        }
    for (int j = 0; j < m; ++j)
        for (int r = 0; r < k; ++r) {
            double s = 0.0;
            for (int c = 0; c < k; ++c) s += C[r * k + c] * (double)work[(int64_t)c * m + j];
            z[(int64_t)r * m + j] = failed ? 0.f : (float)s;
        }
    status[0] = failed ? 1 : 0;
    return SDA_OK;
}

extern "C" int sda_enks_update_host(float* S, int64_t s_st, int64_t s_sp, int nslab, int m, int d, int k, float inflation,
                                    const float* a, const float* z) {
    int rc = enks_update_check(S, s_st, s_sp, nslab, m, d, k, inflation, a, z);
    if (rc != SDA_OK) return rc;
    std::vector<double> P(k);
    for (int sl = 0; sl < nslab; ++sl) {
        float* x = S + (int64_t)sl * s_st;
        for (int c = 0; c < d; ++c) {
            double s = 0.0;
            for (int j = 0; j < m; ++j) s += (double)x[(int64_t)j * s_sp + c];
            const double mean = s / (double)m;
            if (inflation != 1.0f && sl == nslab - 1)
                for (int j = 0; j < m; ++j) x[(int64_t)j * s_sp + c] = enks_inflate(x[(int64_t)j * s_sp + c], (float)mean, inflation);
            for (int r = 0; r < k; ++r) {
                double t = 0.0;
                for (int j = 0; j < m; ++j) t += ((double)x[(int64_t)j * s_sp + c] - mean) * (double)a[(int64_t)r * m + j];
                P[r] = t / (double)(m - 1);
            }
            for (int j = 0; j < m; ++j) {
                double inc = 0.0;
                for (int r = 0; r < k; ++r) inc += P[r] * (double)z[(int64_t)r * m + j];
                float* px = x + (int64_t)j * s_sp + c;
                *px = (float)((double)*px + inc);
            }
        }
    }
    return SDA_OK;
}
#endif  // SDA_HOST_EMU
