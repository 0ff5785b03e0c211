// Linear-Gaussian state space (sda/mcs.py:60-82, DampedSpring, and any x' = A x + b + w, y = H x + c + v with d, k <= 8): the
// simulator, the exact posterior (forward filter, backward sampler, evidence) and the exact eps of the VP-noised trajectory.
// include/sda_hip.h states the formulas and layouts.  One lane owns one state / sequence / sample / trajectory and walks the times
// serially with its state in registers: every loop over components is unrolled to LG_D = 8 with the real d as a guard, so no array
// is indexed at run time.  What all lanes share (A, b, the Kalman tables, the block factor) is read at wave-uniform addresses.
// The arithmetic of a step lives in __host__ __device__ functions; under SDA_HOST_EMU the same functions run as plain loops over
// host arrays (bottom of the file), which is what the CPU tests check.
//
// Stores.  A lane's trajectory is (T + 1) d floats from its neighbour's, so a lane-per-row store touches 64 cache lines per
// instruction.  The sampler and the score stage a tile of LG_TILE / d times per lane in LDS (row stride LG_LD = 65 floats: the 32
// lanes of an LDS write group land on 32 banks) and then write each row's tile as ONE contiguous run of up to 256 bytes, lane =
// float; the score reads its input the same way.
#include "sda_common.hpp"
#include "philox.hpp"

#define LG_D SDA_LGSS_MAXD
#define LG_THREADS 64
#define LG_TILE 64
#define LG_LD 65
#define LG_UNROLL _Pragma("unroll")
#define LG_LOG_2PI 1.83787706640934548356

// the d normals of global row `grow` in draw `draw`: what sda_randn_rows writes to that row of an [rows][d] tensor
__host__ __device__ __forceinline__ void lgss_noise(uint64_t seed, uint64_t grow, int64_t draw, int d, float* z) {
    philox_normal4(0, grow, draw, (uint32_t)seed, (uint32_t)(seed >> 32), z);
    z[4] = z[5] = z[6] = z[7] = 0.f;
    if (d > 4) philox_normal4(1, grow, draw, (uint32_t)seed, (uint32_t)(seed >> 32), z + 4);
}

// ---------------------------------------------------------------- simulator (fp32)
// x <- b + sum_j A[i][j] x[j] (index order, fma), then + sum_{j <= i} Lq[i][j] z[j] (index order, fma)
__host__ __device__ __forceinline__ void lgss_transition(const sda_lgss_model& m, const float* z, float* x) {
    float o[LG_D];
    LG_UNROLL
    for (int i = 0; i < LG_D; ++i) {
        float acc = 0.f;
        if (i < m.d) {
            acc = m.b[i];
            LG_UNROLL
            for (int j = 0; j < LG_D; ++j)
                if (j < m.d) acc = fmaf(m.A[i][j], x[j], acc);
            LG_UNROLL
            for (int j = 0; j < LG_D; ++j)
                if (j <= i) acc = fmaf(m.Lq[i][j], z[j], acc);
        }
        o[i] = acc;
    }
    LG_UNROLL
    for (int i = 0; i < LG_D; ++i) x[i] = o[i];
}

// ---------------------------------------------------------------- float64 pieces shared by the kernels and the host replay
struct LgssDyn {            // what the filter and the sampler need of sda_lgss_model64, by value
    int32_t d, k;
    double A[LG_D * LG_D], b[LG_D], H[LG_D * LG_D], c[LG_D], m0[LG_D];
};

static void lgss_dyn(const sda_lgss_model64* m, LgssDyn& f) {
    f.d = m->d; f.k = m->k;
    for (int i = 0; i < LG_D; ++i) {
        f.b[i] = m->b[i]; f.c[i] = m->c[i]; f.m0[i] = m->m0[i];
        for (int j = 0; j < LG_D; ++j) { f.A[i * LG_D + j] = m->A[i][j]; f.H[i * LG_D + j] = m->H[i][j]; }
    }
}

// table offsets (doubles) inside the slab of one time index
__host__ __device__ __forceinline__ int lgss_tab_stride(int d, int k) { return d * k + 2 * d * d + k * k + 1; }
__host__ __device__ __forceinline__ int lgss_tab_gain(int d, int k) { return 0; }
__host__ __device__ __forceinline__ int lgss_tab_back(int d, int k) { return d * k; }
__host__ __device__ __forceinline__ int lgss_tab_chol(int d, int k) { return d * k + d * d; }
__host__ __device__ __forceinline__ int lgss_tab_innov(int d, int k) { return d * k + 2 * d * d; }
__host__ __device__ __forceinline__ int lgss_tab_logdet(int d, int k) { return d * k + 2 * d * d + k * k; }

// o[c] = base[c] + sum_j M[c][j] v[j] for c < d (M row-major with leading dimension ld, at a wave-uniform address)
__host__ __device__ __forceinline__ void lgss_affine(const double* __restrict__ M, int ld, int d, const double* base, const double* v,
                                                     double* o) {
    LG_UNROLL
    for (int c = 0; c < LG_D; ++c) {
        double acc = 0.0;
        if (c < d) {
            acc = base[c];
            LG_UNROLL
            for (int j = 0; j < LG_D; ++j)
                if (j < d) acc = fma(M[c * ld + j], v[j], acc);
        }
        o[c] = acc;
    }
}

// the filter's mean at one time index: predict (i > 0), then the update where an observation sits.  m: in the mean at i - 1, out at i
__host__ __device__ __forceinline__ void lgss_filter_step(const LgssDyn& f, const double* __restrict__ tab, bool first, bool obs,
                                                          const float* y, double* m, double& logz) {
    const int d = f.d, k = f.k;
    if (!first) {
        double p[LG_D];
        lgss_affine(f.A, LG_D, d, f.b, m, p);
        LG_UNROLL
        for (int c = 0; c < LG_D; ++c) m[c] = p[c];
    }
    if (obs) {
        double v[LG_D], w[LG_D];
        LG_UNROLL
        for (int r = 0; r < LG_D; ++r) {            // innovation v = y - (H m + c)
            double acc = 0.0;
            if (r < k) {
                acc = f.c[r];
                LG_UNROLL
                for (int j = 0; j < LG_D; ++j)
                    if (j < d) acc = fma(f.H[r * LG_D + j], m[j], acc);
                acc = (double)y[r] - acc;
            }
            v[r] = acc;
        }
        const double* Ls = tab + lgss_tab_innov(d, k);
        double quad = 0.0;
        LG_UNROLL
        for (int r = 0; r < LG_D; ++r) {            // w = Ls^-1 v
            double acc = 0.0;
            if (r < k) {
                acc = v[r];
                LG_UNROLL
                for (int j = 0; j < LG_D; ++j)
                    if (j < r) acc = fma(-Ls[r * k + j], w[j], acc);
                acc = acc / Ls[r * k + r];
                quad = fma(acc, acc, quad);
            }
            w[r] = acc;
        }
        logz += -0.5 * (quad + tab[lgss_tab_logdet(d, k)] + (double)k * LG_LOG_2PI);
        const double* K = tab + lgss_tab_gain(d, k);
        LG_UNROLL
        for (int c = 0; c < LG_D; ++c) {
            if (c < d) {
                double acc = m[c];
                LG_UNROLL
                for (int j = 0; j < LG_D; ++j)
                    if (j < k) acc = fma(K[c * k + j], v[j], acc);
                m[c] = acc;
            }
        }
    }
}

// x_T = mean_T + L_T z
__host__ __device__ __forceinline__ void lgss_sample_last(const LgssDyn& f, const double* __restrict__ tab, const double* mean,
                                                          const float* z, double* x) {
    const int d = f.d;
    const double* L = tab + lgss_tab_chol(d, f.k);
    LG_UNROLL
    for (int c = 0; c < LG_D; ++c) {
        double acc = 0.0;
        if (c < d) {
            acc = mean[c];
            LG_UNROLL
            for (int j = 0; j < LG_D; ++j)
                if (j <= c) acc = fma(L[c * d + j], (double)z[j], acc);
        }
        x[c] = acc;
    }
}

// x_i = mean_i + G_i (x_{i+1} - A mean_i - b) + L_i z; x: in x_{i+1}, out x_i
__host__ __device__ __forceinline__ void lgss_sample_step(const LgssDyn& f, const double* __restrict__ tab, const double* mean,
                                                          const float* z, double* x) {
    const int d = f.d;
    double p[LG_D], t[LG_D], o[LG_D];
    lgss_affine(f.A, LG_D, d, f.b, mean, p);
    LG_UNROLL
    for (int c = 0; c < LG_D; ++c) t[c] = x[c] - p[c];
    lgss_affine(tab + lgss_tab_back(d, f.k), d, d, mean, t, o);
    const double* L = tab + lgss_tab_chol(d, f.k);
    LG_UNROLL
    for (int c = 0; c < LG_D; ++c) {
        double acc = o[c];
        if (c < d) {
            LG_UNROLL
            for (int j = 0; j < LG_D; ++j)
                if (j <= c) acc = fma(L[c * d + j], (double)z[j], acc);
        }
        x[c] = acc;
    }
}

// ---- exact score.  prec (doubles): Sinv[d][d], Qinv[d][d], AtQi[d][d] = A^T Q^-1, AtQiA[d][d], mean[(T + 1)][d].
// work (doubles) per time e: L_ee[d][d] (lower; the DIAGONAL holds 1 / L_ee[c][c]) then L_{e+1,e}[d][d].
__host__ __device__ __forceinline__ double lgss_lam_diag(const double* __restrict__ prec, int d, int T, int e, int idx) {
    const int dd = d * d;
    double v = e == 0 ? prec[idx] : prec[dd + idx];
    if (e < T) v += prec[3 * dd + idx];
    return v;
}

// the block Cholesky of mu^2 I + sigma^2 Lambda, block Thomas order; `lane` of `nl` cooperating lanes (host: 0 of 1).  W, Lp: 64
// doubles each that all lanes see (LDS).  LGSS_SYNC() between the phases.
#define LGSS_FACTOR_BODY(LGSS_SYNC)                                                                                                  \
    const int dd = d * d;                                                                                                            \
    const double mu2 = (double)coef[0] * (double)coef[0], s2 = (double)coef[1] * (double)coef[1];                                     \
    for (int e = 0; e <= T; ++e) {                                                                                                   \
        for (int idx = lane; idx < dd; idx += nl) {                                                                                  \
            const int r = idx / d, c = idx - r * d;                                                                                  \
            double v = s2 * lgss_lam_diag(prec, d, T, e, idx) + (r == c ? mu2 : 0.0);                                                 \
            if (e > 0)                                                                                                               \
                for (int q = 0; q < d; ++q) v -= Lp[r * d + q] * Lp[c * d + q];                                                      \
            W[idx] = v;                                                                                                              \
        }                                                                                                                            \
        LGSS_SYNC();                                                                                                                 \
        for (int j = 0; j < d; ++j) {                                                                                                \
            if (lane == 0) {                                                                                                         \
                double s = W[j * d + j];                                                                                             \
                for (int q = 0; q < j; ++q) s -= W[j * d + q] * W[j * d + q];                                                        \
                W[j * d + j] = sqrt(s);                                                                                              \
            }                                                                                                                        \
            LGSS_SYNC();                                                                                                             \
            for (int r = j + 1 + lane; r < d; r += nl) {                                                                             \
                double s = W[r * d + j];                                                                                             \
                for (int q = 0; q < j; ++q) s -= W[r * d + q] * W[j * d + q];                                                        \
                W[r * d + j] = s / W[j * d + j];                                                                                     \
            }                                                                                                                        \
            LGSS_SYNC();                                                                                                             \
        }                                                                                                                            \
        double* slab = work + (int64_t)e * 2 * dd;                                                                                   \
        for (int idx = lane; idx < dd; idx += nl) {                                                                                  \
            const int r = idx / d, c = idx - r * d;                                                                                  \
            slab[idx] = r == c ? 1.0 / W[idx] : (c < r ? W[idx] : 0.0);                                                              \
        }                                                                                                                            \
        for (int r = lane; r < d; r += nl) {        /* X L^T = E = -sigma^2 Q^-1 A = -sigma^2 AtQi^T, row r */                        \
            for (int c = 0; c < d; ++c) {                                                                                            \
                double s = e < T ? -s2 * prec[2 * dd + c * d + r] : 0.0;                                                             \
                for (int q = 0; q < c; ++q) s -= Lp[r * d + q] * W[c * d + q];                                                       \
                Lp[r * d + c] = s / W[c * d + c];                                                                                    \
                slab[dd + r * d + c] = Lp[r * d + c];                                                                                \
            }                                                                                                                        \
        }                                                                                                                            \
        LGSS_SYNC();                                                                                                                 \
    }

// forward sweep at time e: y_e = L_ee^-1 (r_e - L_{e,e-1} y_{e-1}); y: in y_{e-1}, out y_e
__host__ __device__ __forceinline__ void lgss_score_fwd(const double* __restrict__ work, int d, int e, const double* r, double* y) {
    const int dd = d * d;
    double rhs[LG_D];
    LG_UNROLL
    for (int c = 0; c < LG_D; ++c) rhs[c] = r[c];
    if (e > 0) {
        const double* Lp = work + (int64_t)(e - 1) * 2 * dd + dd;
        LG_UNROLL
        for (int c = 0; c < LG_D; ++c) {
            if (c < d) {
                double acc = rhs[c];
                LG_UNROLL
                for (int j = 0; j < LG_D; ++j)
                    if (j < d) acc = fma(-Lp[c * d + j], y[j], acc);
                rhs[c] = acc;
            }
        }
    }
    const double* L = work + (int64_t)e * 2 * dd;
    LG_UNROLL
    for (int c = 0; c < LG_D; ++c) {
        double acc = 0.0;
        if (c < d) {
            acc = rhs[c];
            LG_UNROLL
            for (int j = 0; j < LG_D; ++j)
                if (j < c) acc = fma(-L[c * d + j], y[j], acc);
            acc *= L[c * d + c];
        }
        y[c] = acc;
    }
}

// backward sweep at time e: u_e = L_ee^-T (y_e - L_{e+1,e}^T u_{e+1}); un = u_{e+1} (ignored at e = T)
__host__ __device__ __forceinline__ void lgss_score_bwd(const double* __restrict__ work, int d, int T, int e, const double* y,
                                                        const double* un, double* u) {
    const int dd = d * d;
    const double* L = work + (int64_t)e * 2 * dd;
    const double* Ln = L + dd;
    double rhs[LG_D];
    LG_UNROLL
    for (int c = 0; c < LG_D; ++c) rhs[c] = y[c];
    if (e < T) {
        LG_UNROLL
        for (int c = 0; c < LG_D; ++c) {
            if (c < d) {
                double acc = rhs[c];
                LG_UNROLL
                for (int j = 0; j < LG_D; ++j)
                    if (j < d) acc = fma(-Ln[j * d + c], un[j], acc);
                rhs[c] = acc;
            }
        }
    }
    LG_UNROLL
    for (int cc = 0; cc < LG_D; ++cc) {
        const int c = LG_D - 1 - cc;
        double acc = 0.0;
        if (c < d) {
            acc = rhs[c];
            LG_UNROLL
            for (int j = 0; j < LG_D; ++j)
                if (j > c && j < d) acc = fma(-L[j * d + c], u[j], acc);
            acc *= L[c * d + c];
        }
        u[c] = acc;
    }
}

// eps_e = sigma (Lambda_ee u_e - AtQi u_{e+1} - AtQi^T u_{e-1})
__host__ __device__ __forceinline__ void lgss_score_out(const double* __restrict__ prec, int d, int T, int e, double sigma,
                                                        const double* up, const double* u, const double* un, double* eps) {
    const int dd = d * d;
    LG_UNROLL
    for (int c = 0; c < LG_D; ++c) {
        double acc = 0.0;
        if (c < d) {
            LG_UNROLL
            for (int j = 0; j < LG_D; ++j)
                if (j < d) acc = fma(lgss_lam_diag(prec, d, T, e, c * d + j), u[j], acc);
            if (e < T) {
                LG_UNROLL
                for (int j = 0; j < LG_D; ++j)
                    if (j < d) acc = fma(-prec[2 * dd + c * d + j], un[j], acc);
            }
            if (e > 0) {
                LG_UNROLL
                for (int j = 0; j < LG_D; ++j)
                    if (j < d) acc = fma(-prec[2 * dd + j * d + c], up[j], acc);
            }
        }
        eps[c] = sigma * acc;
    }
}

// ---------------------------------------------------------------- host: the Kalman / backward tables (float64, no device access)
static bool lg_chol(const double* S, int n, double* L) {       // lower factor of a symmetric n x n matrix; false: not positive definite
    for (int i = 0; i < n * n; ++i) L[i] = 0.0;
    for (int j = 0; j < n; ++j) {
        double s = S[j * n + j];
        for (int q = 0; q < j; ++q) s -= L[j * n + q] * L[j * n + q];
        if (!(s > 0.0) || !(s < INFINITY)) return false;
        L[j * n + j] = sqrt(s);
        for (int r = j + 1; r < n; ++r) {
            double t = S[r * n + j];
            for (int q = 0; q < j; ++q) t -= L[r * n + q] * L[j * n + q];
            L[r * n + j] = t / L[j * n + j];
        }
    }
    return true;
}

static void lg_chol_solve(const double* L, int n, double* v) {     // v <- (L L^T)^-1 v
    for (int r = 0; r < n; ++r) {
        double s = v[r];
        for (int q = 0; q < r; ++q) s -= L[r * n + q] * v[q];
        v[r] = s / L[r * n + r];
    }
    for (int r = n - 1; r >= 0; --r) {
        double s = v[r];
        for (int q = r + 1; q < n; ++q) s -= L[q * n + r] * v[q];
        v[r] = s / L[r * n + r];
    }
}

// C (n x p) = X (n x m) Y (m x p), or with Y transposed (Y given p x m)
static void lg_mm(const double* X, const double* Y, int n, int m, int p, bool yt, double* C) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < p; ++j) {
            double s = 0.0;
            for (int q = 0; q < m; ++q) s += X[i * m + q] * (yt ? Y[j * m + q] : Y[q * p + j]);
            C[i * p + j] = s;
        }
}

static void lg_sym(double* P, int n) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j) P[i * n + j] = P[j * n + i] = 0.5 * (P[i * n + j] + P[j * n + i]);
}

static int lgss_model64_check(const sda_lgss_model64* m) {
    if (!m || m->d < 1 || m->d > LG_D || m->k < 1 || m->k > LG_D || !(m->sigma > 0.0)) return SDA_E_BADARG;
    return SDA_OK;
}

extern "C" int64_t sda_lgss_table_doubles(int d, int k, int T) {
    if (d < 1 || d > LG_D || k < 1 || k > LG_D || T < 0) return SDA_E_BADARG;
    return (int64_t)(T + 1) * lgss_tab_stride(d, k);
}

extern "C" int sda_lgss_tables(const sda_lgss_model64* m, int step, int N, double* table) {
    int rc = lgss_model64_check(m);
    if (rc != SDA_OK) return rc;
    if (!table || step < 1 || N < 1 || (int64_t)(N - 1) * step > 0x3fffffff) return SDA_E_BADARG;
    const int d = m->d, k = m->k, T = (N - 1) * step;
    double A[64], Q[64], H[64], P[64], t1[64], t2[64], L[64];
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) { A[i * d + j] = m->A[i][j]; Q[i * d + j] = m->Q[i][j]; P[i * d + j] = m->P0[i][j]; }
    for (int i = 0; i < k; ++i)
        for (int j = 0; j < d; ++j) H[i * d + j] = m->H[i][j];
    lg_sym(Q, d);
    lg_sym(P, d);
    if (!lg_chol(Q, d, L) || !lg_chol(P, d, L)) return SDA_E_BADARG;
    const int stride = lgss_tab_stride(d, k);
    for (int i = 0; i <= T; ++i) {
        double* tab = table + (int64_t)i * stride;
        for (int q = 0; q < stride; ++q) tab[q] = 0.0;
        if (i % step == 0) {
            double PHt[64], S[64], Ls[64];
            lg_mm(P, H, d, d, k, true, PHt);                     // d x k
            lg_mm(H, PHt, k, d, k, false, S);
            for (int r = 0; r < k; ++r) S[r * k + r] += m->sigma * m->sigma;
            lg_sym(S, k);
            if (!lg_chol(S, k, Ls)) return SDA_E_BADARG;
            double logdet = 0.0;
            for (int r = 0; r < k; ++r) logdet += 2.0 * log(Ls[r * k + r]);
            double* K = tab + lgss_tab_gain(d, k);
            for (int r = 0; r < d; ++r) {                        // K = P H^T S^-1, row by row (S symmetric)
                for (int q = 0; q < k; ++q) K[r * k + q] = PHt[r * k + q];
                lg_chol_solve(Ls, k, K + r * k);
            }
            for (int q = 0; q < k * k; ++q) tab[lgss_tab_innov(d, k) + q] = Ls[q];
            tab[lgss_tab_logdet(d, k)] = logdet;
            // Joseph form: P <- (I - K H) P (I - K H)^T + sigma^2 K K^T
            double IKH[64];
            lg_mm(K, H, d, k, d, false, IKH);
            for (int q = 0; q < d * d; ++q) IKH[q] = -IKH[q];
            for (int r = 0; r < d; ++r) IKH[r * d + r] += 1.0;
            lg_mm(IKH, P, d, d, d, false, t1);
            lg_mm(t1, IKH, d, d, d, true, t2);
            lg_mm(K, K, d, k, d, true, t1);
            for (int q = 0; q < d * d; ++q) P[q] = t2[q] + m->sigma * m->sigma * t1[q];
            lg_sym(P, d);
        }
        double* Lc = tab + lgss_tab_chol(d, k);
        if (i == T) {
            if (!lg_chol(P, d, Lc)) return SDA_E_BADARG;
            break;
        }
        double Pp[64], PAt[64], IGA[64], C[64];
        lg_mm(A, P, d, d, d, false, t1);
        lg_mm(t1, A, d, d, d, true, Pp);
        for (int q = 0; q < d * d; ++q) Pp[q] += Q[q];
        lg_sym(Pp, d);
        if (!lg_chol(Pp, d, L)) return SDA_E_BADARG;
        double* G = tab + lgss_tab_back(d, k);
        lg_mm(P, A, d, d, d, true, PAt);
        for (int r = 0; r < d; ++r) {                            // G = P A^T Pp^-1
            for (int q = 0; q < d; ++q) G[r * d + q] = PAt[r * d + q];
            lg_chol_solve(L, d, G + r * d);
        }
        // P - G A P in its Joseph form (I - G A) P (I - G A)^T + G Q G^T
        lg_mm(G, A, d, d, d, false, IGA);
        for (int q = 0; q < d * d; ++q) IGA[q] = -IGA[q];
        for (int r = 0; r < d; ++r) IGA[r * d + r] += 1.0;
        lg_mm(IGA, P, d, d, d, false, t1);
        lg_mm(t1, IGA, d, d, d, true, C);
        lg_mm(G, Q, d, d, d, false, t1);
        lg_mm(t1, G, d, d, d, true, t2);
        for (int q = 0; q < d * d; ++q) C[q] += t2[q];
        lg_sym(C, d);
        if (!lg_chol(C, d, Lc)) return SDA_E_BADARG;
        for (int q = 0; q < d * d; ++q) P[q] = Pp[q];
    }
    return SDA_OK;
}

static int lgss_model_check(const sda_lgss_model* m) { return !m || m->d < 1 || m->d > LG_D ? SDA_E_BADARG : SDA_OK; }

static int lgss_advance_check(const sda_lgss_model* model, const float* x_in, int64_t in_sp, int m, int transitions, const float* out,
                              int64_t out_st, int64_t out_sp, int64_t row0, int64_t draw0) {
    int rc = lgss_model_check(model);
    if (rc != SDA_OK) return rc;
    if (!x_in || !out || m < 1 || transitions < 1 || row0 < 0 || draw0 < 0 || in_sp < model->d || out_sp < model->d || out_st < 0)
        return SDA_E_BADARG;
    return SDA_OK;
}

static int lgss_filter_check(const sda_lgss_model64* m, const void* table, int step, int N, const void* y, int B, const void* mean,
                             const void* logz) {
    int rc = lgss_model64_check(m);
    if (rc != SDA_OK) return rc;
    if (!table || !y || !mean || !logz || step < 1 || N < 1 || B < 1 || (int64_t)(N - 1) * step > 0x3fffffff) return SDA_E_BADARG;
    return SDA_OK;
}

static int lgss_sample_check(const sda_lgss_model64* m, const void* table, const void* mean, int T, int B, int M, int64_t row0,
                             int64_t draw0, const void* out) {
    int rc = lgss_model64_check(m);
    if (rc != SDA_OK) return rc;
    if (!table || !mean || !out || T < 0 || B < 1 || M < 1 || row0 < 0 || draw0 < 0) return SDA_E_BADARG;
    if ((int64_t)B * M > 0x7fffffff - LG_THREADS) return SDA_E_UNSUPPORTED;
    return SDA_OK;
}

static int lgss_score_check(int d, int T, const void* prec, const void* coef, const void* work) {
    if (d < 1 || d > LG_D || T < 0 || !prec || !coef || !work) return SDA_E_BADARG;
    return SDA_OK;
}

extern "C" int64_t sda_lgss_score_doubles(int d, int T, int which) {
    if (d < 1 || d > LG_D || T < 0 || which < 0 || which > 1) return SDA_E_BADARG;
    return which == 0 ? 4 * d * d + (int64_t)(T + 1) * d : (int64_t)(T + 1) * 2 * d * d;
}

#ifndef SDA_HOST_EMU
// ---------------------------------------------------------------- device kernels
struct LgssAdvArgs {
    sda_lgss_model model;
    const float* x_in; int64_t in_sp;
    float* out; int64_t out_st, out_sp; int32_t every, m, transitions;
    uint64_t seed; int64_t row0, draw0;
};

__global__ __launch_bounds__(256) void lgss_advance_kernel(LgssAdvArgs a) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.m) return;
    const int d = a.model.d;
    float x[LG_D], z[LG_D];
    LG_UNROLL
    for (int c = 0; c < LG_D; ++c) x[c] = c < d ? a.x_in[j * a.in_sp + c] : 0.f;
    for (int t = 0; t < a.transitions; ++t) {
        lgss_noise(a.seed, (uint64_t)(a.row0 + j), a.draw0 + t, d, z);
        lgss_transition(a.model, z, x);
        if (a.every) {
            LG_UNROLL
            for (int c = 0; c < LG_D; ++c)
                if (c < d) a.out[t * a.out_st + j * a.out_sp + c] = x[c];
        }
    }
    if (!a.every) {
        LG_UNROLL
        for (int c = 0; c < LG_D; ++c)
            if (c < d) a.out[j * a.out_sp + c] = x[c];
    }
}

extern "C" int sda_lgss_advance(const sda_lgss_model* model, const float* x_in, int64_t in_sp, int m, int transitions, int every,
                                float* out, int64_t out_st, int64_t out_sp, uint64_t seed, int64_t row0, int64_t draw0, void* stream) {
    int rc = lgss_advance_check(model, x_in, in_sp, m, transitions, out, out_st, out_sp, row0, draw0);
    if (rc != SDA_OK) return rc;
    LgssAdvArgs a;
    a.model = *model;
    a.x_in = x_in; a.in_sp = in_sp;
    a.out = out; a.out_st = every ? out_st : 0; a.out_sp = out_sp; a.every = every ? 1 : 0; a.m = m; a.transitions = transitions;
    a.seed = seed; a.row0 = row0; a.draw0 = draw0;
    hipLaunchKernelGGL(lgss_advance_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return sda_launch_status();
}

// one observation sequence per lane
__global__ __launch_bounds__(LG_THREADS) void lgss_filter_kernel(LgssDyn f, const double* __restrict__ table, int step, int N,
                                                                 const float* __restrict__ y, int B, double* __restrict__ mean,
                                                                 double* __restrict__ logz) {
    const int s = blockIdx.x * LG_THREADS + threadIdx.x;
    if (s >= B) return;
    const int d = f.d, k = f.k, T = (N - 1) * step, stride = lgss_tab_stride(d, k);
    double m[LG_D], lz = 0.0;
    LG_UNROLL
    for (int c = 0; c < LG_D; ++c) m[c] = c < d ? f.m0[c] : 0.0;
    int next = 0, j = 0;                               // the next observed time index and its observation
    for (int i = 0; i <= T; ++i) {
        const bool obs = i == next;
        float yv[LG_D];
        LG_UNROLL
        for (int r = 0; r < LG_D; ++r) yv[r] = obs && r < k ? y[((int64_t)s * N + j) * k + r] : 0.f;
        lgss_filter_step(f, table + (int64_t)i * stride, i == 0, obs, yv, m, lz);
        if (obs) { next += step; ++j; }
        LG_UNROLL
        for (int c = 0; c < LG_D; ++c)
            if (c < d) mean[((int64_t)s * (T + 1) + i) * d + c] = m[c];
    }
    logz[s] = lz;
}

extern "C" int sda_lgss_filter(const sda_lgss_model64* model, const double* table, int step, int N, const float* y, int B, double* mean,
                               double* logz, void* stream) {
    int rc = lgss_filter_check(model, table, step, N, y, B, mean, logz);
    if (rc != SDA_OK) return rc;
    LgssDyn f;
    lgss_dyn(model, f);
    hipLaunchKernelGGL(lgss_filter_kernel, dim3((unsigned)((B + LG_THREADS - 1) / LG_THREADS)), dim3(LG_THREADS), 0, (hipStream_t)stream,
                       f, table, step, N, y, B, mean, logz);
    return sda_launch_status();
}

// the workgroup's rows [row0, row0 + rows) x columns [col0, col0 + n) of a [..][width] fp32 tensor <-> the LDS tile, each row one
// contiguous run (n <= 64: lane = float).  Every lane of the workgroup calls these; the caller puts the barriers.
__device__ __forceinline__ void lgss_tile_store(const float* tile, float* __restrict__ out, int64_t row0, int rows, int64_t width,
                                                int64_t col0, int n) {
    const int lane = threadIdx.x;
    if (lane < n)
        for (int r = 0; r < rows; ++r) out[(row0 + r) * width + col0 + lane] = tile[r * LG_LD + lane];
}
__device__ __forceinline__ void lgss_tile_load(float* tile, const float* __restrict__ in, int64_t row0, int rows, int64_t width,
                                               int64_t col0, int n) {
    const int lane = threadIdx.x;
    if (lane < n)
        for (int r = 0; r < rows; ++r) tile[r * LG_LD + lane] = in[(row0 + r) * width + col0 + lane];
}

// one posterior sample per lane, times T down to 0
__global__ __launch_bounds__(LG_THREADS) void lgss_sample_kernel(LgssDyn f, const double* __restrict__ table,
                                                                 const double* __restrict__ mean, int T, int total, int M, uint64_t seed,
                                                                 int64_t row0, int64_t draw0, float* __restrict__ out) {
    __shared__ float tile[LG_THREADS * LG_LD];
    const int lane = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * LG_THREADS;
    const int64_t idx = first + lane;
    const bool live = idx < total;
    const int rows = total - first < LG_THREADS ? (int)(total - first) : LG_THREADS;
    const int d = f.d, stride = lgss_tab_stride(d, f.k);
    const int per = LG_TILE / d;                       // times per tile
    const double* mrow = mean + (live ? idx / M : 0) * (int64_t)(T + 1) * d;
    double x[LG_D];
    LG_UNROLL
    for (int c = 0; c < LG_D; ++c) x[c] = 0.0;
    for (int hi = T; hi >= 0; hi -= per) {
        const int lo = hi - per + 1 > 0 ? hi - per + 1 : 0;
        if (live) {
            for (int i = hi; i >= lo; --i) {
                float z[LG_D];
                double mi[LG_D];
                lgss_noise(seed, (uint64_t)(row0 + idx), draw0 + i, d, z);
                LG_UNROLL
                for (int c = 0; c < LG_D; ++c) mi[c] = c < d ? mrow[(int64_t)i * d + c] : 0.0;
                const double* tab = table + (int64_t)i * stride;
                if (i == T) lgss_sample_last(f, tab, mi, z, x); else lgss_sample_step(f, tab, mi, z, x);
                LG_UNROLL
                for (int c = 0; c < LG_D; ++c)
                    if (c < d) tile[lane * LG_LD + (i - lo) * d + c] = (float)x[c];
            }
        }
        __syncthreads();
        lgss_tile_store(tile, out, first, rows, (int64_t)(T + 1) * d, (int64_t)lo * d, (hi - lo + 1) * d);
        __syncthreads();
    }
}

extern "C" int sda_lgss_sample(const sda_lgss_model64* model, const double* table, const double* mean, int T, int B, int M, uint64_t seed,
                               int64_t row0, int64_t draw0, float* out, void* stream) {
    int rc = lgss_sample_check(model, table, mean, T, B, M, row0, draw0, out);
    if (rc != SDA_OK) return rc;
    LgssDyn f;
    lgss_dyn(model, f);
    const int total = B * M;
    hipLaunchKernelGGL(lgss_sample_kernel, dim3((unsigned)((total + LG_THREADS - 1) / LG_THREADS)), dim3(LG_THREADS), 0,
                       (hipStream_t)stream, f, table, mean, T, total, M, seed, row0, draw0, out);
    return sda_launch_status();
}

// ONE wave: lane (r, c) of up to 64 forms its entry of a block, the columns of the d x d Cholesky follow one another
__global__ __launch_bounds__(LG_THREADS) void lgss_score_factor_kernel(int d, int T, const double* __restrict__ prec,
                                                                       const float* __restrict__ coef, double* __restrict__ work) {
    __shared__ double W[LG_D * LG_D], Lp[LG_D * LG_D];
    const int lane = threadIdx.x, nl = LG_THREADS;
    LGSS_FACTOR_BODY(__syncthreads)
}

extern "C" int sda_lgss_score_factor(int d, int T, const double* prec, const float* coef, double* work, void* stream) {
    int rc = lgss_score_check(d, T, prec, coef, work);
    if (rc != SDA_OK) return rc;
    hipLaunchKernelGGL(lgss_score_factor_kernel, dim3(1), dim3(LG_THREADS), 0, (hipStream_t)stream, d, T, prec, coef, work);
    return sda_launch_status();
}

// one trajectory per lane: forward sweep (y to ywork[(e d + c) n + row], coalesced), then backward sweep and the product with Lambda
__global__ __launch_bounds__(LG_THREADS) void lgss_score_kernel(int d, int T, const double* __restrict__ prec,
                                                                const float* __restrict__ coef, const double* __restrict__ work,
                                                                const float* __restrict__ x, int n, int zero_mean,
                                                                double* __restrict__ ywork, float* __restrict__ out) {
    __shared__ float tile[LG_THREADS * LG_LD];
    const int lane = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * LG_THREADS;
    const int64_t row = first + lane;
    const bool live = row < n;
    const int rows = n - first < LG_THREADS ? (int)(n - first) : LG_THREADS;
    const int per = LG_TILE / d;
    const int64_t width = (int64_t)(T + 1) * d;
    const double mu = zero_mean ? 0.0 : (double)coef[0], sigma = (double)coef[1];
    const double* pm = prec + 4 * d * d;
    double y[LG_D];
    LG_UNROLL
    for (int c = 0; c < LG_D; ++c) y[c] = 0.0;
    for (int lo = 0; lo <= T; lo += per) {
        const int hi = lo + per - 1 < T ? lo + per - 1 : T;
        lgss_tile_load(tile, x, first, rows, width, (int64_t)lo * d, (hi - lo + 1) * d);
        __syncthreads();
        if (live) {
            for (int e = lo; e <= hi; ++e) {
                double r[LG_D];
                LG_UNROLL
                for (int c = 0; c < LG_D; ++c)
                    r[c] = c < d ? fma(-mu, pm[(int64_t)e * d + c], (double)tile[lane * LG_LD + (e - lo) * d + c]) : 0.0;
                lgss_score_fwd(work, d, e, r, y);
                LG_UNROLL
                for (int c = 0; c < LG_D; ++c)
                    if (c < d) ywork[((int64_t)e * d + c) * n + row] = y[c];
            }
        }
        __syncthreads();
    }
    double up[LG_D], u[LG_D], un[LG_D], eps[LG_D];
    LG_UNROLL
    for (int c = 0; c < LG_D; ++c) up[c] = u[c] = un[c] = 0.0;
    if (live) lgss_score_bwd(work, d, T, T, y, un, u);         // u_T from y_T, still in registers
    for (int hi = T; hi >= 0; hi -= per) {
        const int lo = hi - per + 1 > 0 ? hi - per + 1 : 0;
        if (live) {
            for (int e = hi; e >= lo; --e) {
                if (e > 0) {
                    LG_UNROLL
                    for (int c = 0; c < LG_D; ++c) y[c] = c < d ? ywork[((int64_t)(e - 1) * d + c) * n + row] : 0.0;
                    lgss_score_bwd(work, d, T, e - 1, y, u, up);
                }
                lgss_score_out(prec, d, T, e, sigma, up, u, un, eps);
                LG_UNROLL
                for (int c = 0; c < LG_D; ++c) {
                    if (c < d) tile[lane * LG_LD + (e - lo) * d + c] = (float)eps[c];
                    un[c] = u[c];
                    u[c] = up[c];
                }
            }
        }
        __syncthreads();
        lgss_tile_store(tile, out, first, rows, width, (int64_t)lo * d, (hi - lo + 1) * d);
        __syncthreads();
    }
}

extern "C" int sda_lgss_score(int d, int T, const double* prec, const float* coef, const double* work, const float* x, int n,
                              int zero_mean, double* ywork, float* out, void* stream) {
    int rc = lgss_score_check(d, T, prec, coef, work);
    if (rc != SDA_OK) return rc;
    if (!x || !ywork || !out || n < 1) return SDA_E_BADARG;
    hipLaunchKernelGGL(lgss_score_kernel, dim3((unsigned)((n + LG_THREADS - 1) / LG_THREADS)), dim3(LG_THREADS), 0, (hipStream_t)stream,
                       d, T, prec, coef, work, x, n, zero_mean, ywork, out);
    return sda_launch_status();
}

#else  // SDA_HOST_EMU
// ---------------------------------------------------------------- CPU replay (tests only; libsda_emu.so): the same functions as plain
// loops over HOST arrays, without the LDS staging
extern "C" int sda_lgss_advance_host(const sda_lgss_model* model, const float* x_in, int64_t in_sp, int m, int transitions, int every,
                                     float* out, int64_t out_st, int64_t out_sp, uint64_t seed, int64_t row0, int64_t draw0) {
    int rc = lgss_advance_check(model, x_in, in_sp, m, transitions, out, out_st, out_sp, row0, draw0);
    if (rc != SDA_OK) return rc;
    const int d = model->d;
    for (int j = 0; j < m; ++j) {
        float x[LG_D] = {}, z[LG_D];
        for (int c = 0; c < d; ++c) x[c] = x_in[j * in_sp + c];
        for (int t = 0; t < transitions; ++t) {
            lgss_noise(seed, (uint64_t)(row0 + j), draw0 + t, d, z);
            lgss_transition(*model, z, x);
            if (every)
                for (int c = 0; c < d; ++c) out[t * out_st + j * out_sp + c] = x[c];
        }
        if (!every)
            for (int c = 0; c < d; ++c) out[j * out_sp + c] = x[c];
    }
    return SDA_OK;
}

extern "C" int sda_lgss_filter_host(const sda_lgss_model64* model, const double* table, int step, int N, const float* y, int B,
                                    double* mean, double* logz) {
    int rc = lgss_filter_check(model, table, step, N, y, B, mean, logz);
    if (rc != SDA_OK) return rc;
    LgssDyn f;
    lgss_dyn(model, f);
    const int d = f.d, k = f.k, T = (N - 1) * step, stride = lgss_tab_stride(d, k);
    for (int s = 0; s < B; ++s) {
        double m[LG_D] = {}, lz = 0.0;
        for (int c = 0; c < d; ++c) m[c] = f.m0[c];
        for (int i = 0; i <= T; ++i) {
            float yv[LG_D] = {};
            const bool obs = i % step == 0;
            if (obs)
                for (int r = 0; r < k; ++r) yv[r] = y[((int64_t)s * N + i / step) * k + r];
            lgss_filter_step(f, table + (int64_t)i * stride, i == 0, obs, yv, m, lz);
            for (int c = 0; c < d; ++c) mean[((int64_t)s * (T + 1) + i) * d + c] = m[c];
        }
        logz[s] = lz;
    }
    return SDA_OK;
}

extern "C" int sda_lgss_sample_host(const sda_lgss_model64* model, const double* table, const double* mean, int T, int B, int M,
                                    uint64_t seed, int64_t row0, int64_t draw0, float* out) {
    int rc = lgss_sample_check(model, table, mean, T, B, M, row0, draw0, out);
    if (rc != SDA_OK) return rc;
    LgssDyn f;
    lgss_dyn(model, f);
    const int d = f.d, stride = lgss_tab_stride(d, f.k);
    for (int64_t idx = 0; idx < (int64_t)B * M; ++idx) {
        double x[LG_D] = {};
        for (int i = T; i >= 0; --i) {
            float z[LG_D];
            double mi[LG_D] = {};
            lgss_noise(seed, (uint64_t)(row0 + idx), draw0 + i, d, z);
            for (int c = 0; c < d; ++c) mi[c] = mean[((idx / M) * (T + 1) + i) * d + c];
            const double* tab = table + (int64_t)i * stride;
            if (i == T) lgss_sample_last(f, tab, mi, z, x); else lgss_sample_step(f, tab, mi, z, x);
            for (int c = 0; c < d; ++c) out[(idx * (T + 1) + i) * d + c] = (float)x[c];
        }
    }
    return SDA_OK;
}

static inline void lgss_no_sync() {}

extern "C" int sda_lgss_score_factor_host(int d, int T, const double* prec, const float* coef, double* work) {
    int rc = lgss_score_check(d, T, prec, coef, work);
    if (rc != SDA_OK) return rc;
    double W[LG_D * LG_D], Lp[LG_D * LG_D];
    const int lane = 0, nl = 1;
    LGSS_FACTOR_BODY(lgss_no_sync)
    return SDA_OK;
}

extern "C" int sda_lgss_score_host(int d, int T, const double* prec, const float* coef, const double* work, const float* x, int n,
                                   int zero_mean, double* ywork, float* out) {
    int rc = lgss_score_check(d, T, prec, coef, work);
    if (rc != SDA_OK) return rc;
    if (!x || !ywork || !out || n < 1) return SDA_E_BADARG;
    const double mu = zero_mean ? 0.0 : (double)coef[0], sigma = (double)coef[1];
    const double* pm = prec + 4 * d * d;
    for (int64_t row = 0; row < n; ++row) {
        double y[LG_D] = {}, up[LG_D] = {}, u[LG_D] = {}, un[LG_D] = {}, eps[LG_D];
        for (int e = 0; e <= T; ++e) {
            double r[LG_D] = {};
            for (int c = 0; c < d; ++c) r[c] = fma(-mu, pm[(int64_t)e * d + c], (double)x[(row * (T + 1) + e) * d + c]);
            lgss_score_fwd(work, d, e, r, y);
            for (int c = 0; c < d; ++c) ywork[((int64_t)e * d + c) * n + row] = y[c];
        }
        lgss_score_bwd(work, d, T, T, y, un, u);
        for (int e = T; e >= 0; --e) {
            if (e > 0) {
                for (int c = 0; c < LG_D; ++c) y[c] = c < d ? ywork[((int64_t)(e - 1) * d + c) * n + row] : 0.0;
                lgss_score_bwd(work, d, T, e - 1, y, u, up);
            }
            lgss_score_out(prec, d, T, e, sigma, up, u, un, eps);
            for (int c = 0; c < LG_D; ++c) {
                if (c < d) out[(row * (T + 1) + e) * d + c] = (float)eps[c];
                un[c] = u[c];
                u[c] = up[c];
            }
        }
    }
    return SDA_OK;
}
#endif  // SDA_HOST_EMU
