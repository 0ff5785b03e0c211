// Kolmogorov flow (the simulator behind sda/mcs.py:244-338) on the device: an incompressible Navier-Stokes sub-step on a periodic
// staggered N x N grid, forward Euler on the explicit terms (van-Leer-limited Lax-Wendroff advection, 5-point diffusion,
// Kolmogorov forcing with linear drag), then an exact pressure projection.  DESIGN.md section 5 states the scheme; the NumPy
// restatement tests/kflow_ref.py is what the kernels are checked against.
//
// A sub-step is five launches:
//   kflow_explicit_kernel            u*, v* from one read of the state (LDS tile with a halo of 2 on every side)
//   kflow_gemm_kernel<0, 1>          T1 = Hm div(u*, v*)          the divergence is formed in the loader
//   kflow_gemm_kernel<1, 0>          T2 = (T1 Hm) o 1/(lam_a + lam_b)   the scale (0 for the mean mode) in the epilogue
//   kflow_gemm_kernel<0, 0>          T3 = Hm T2
//   kflow_gemm_kernel<1, 1>          q = T3 Hm, and u' = u* - dq/dx, v' = v* - dq/dy in the epilogue
// Hm[a][b] = (cos(2 pi a b / N) + sin(2 pi a b / N)) / sqrt(N) is real, symmetric and its own inverse, and the symmetric circulant
// Laplacian is diagonal in it, so the solve is four dense N x N x N products on v_mfma_f32_16x16x4_f32 with one constant matrix
// that stays in L2.  No FFT library, no power-of-two restriction: N % 16 == 0, 16 <= N <= 512.
//
// The gradient epilogue needs q one row and one column past its 64 x 64 tile.  The last product therefore keeps three
// accumulators per fragment: q, q shifted by one row (the A rows one further) and q shifted by one column (the B columns one
// further).  All three are the same blocked fma chains a neighbouring tile computes for the same element, so the values that
// meet at a tile edge are bitwise equal and the projection is as exact at the edges as inside.
//
// The adjoint (opt-in, KolmogorovFlow(grad='device')).  D is a backward difference and G a forward one, so G = -D^T; L and Hm are
// symmetric; hence P = I - G L^-1 D is its own transpose and the four product launches above ARE the adjoint of the projection.
// The one new kernel is kflow_explicit_vjp_kernel, the vector-Jacobian product of kflow_explicit_kernel at a stored state, in
// gather form (no atomics: bitwise reproducible, independent of the batch).  A transition runs backwards as: recompute its
// sub-step states with the forward launches (bitwise the states the forward pass went through), then per sub-step, last to first,
// g <- P g (four launches) and g <- E'(x_s)^T g (one launch).
#include "sda_common.hpp"

#define KF_THREADS 256
#define KF_T 16             // explicit kernel: cells per tile side
#define KF_HALO 2           // face i - 1 reads c[i - 2]; the `cpp` tap reads c[i + 2]
#define KF_LT (KF_T + 2 * KF_HALO)
#define KF_VH 3             // VJP, state halo: cell i is the cpp tap of face i - 2, whose cm tap is c[i - 3]; face i + 1 reads cpp = c[i + 3]
#define KF_VG 2             // VJP, cotangent halo: the cotangent of face i - 2 reads g[i - 2], that of face i + 1 reads g[i + 2]
#define KF_VLT (KF_T + 2 * KF_VH)
#define KF_VGT (KF_T + 2 * KF_VG)
#define KF_VFL (KF_T + 3)   // VJP, faces along the flux axis: -2 .. KF_T
#define KF_VFC (KF_T + 1)   // VJP, faces across it: -1 .. KF_T - 1 (line -1 reaches the other field through the advecting velocity)
#define KF_VFN (KF_VFL * KF_VFC)
#define KF_TILE 64          // product kernels: output tile side
#define KF_KC 16            // k-chunk
#define KF_SK 80            // LDS row stride of a [k][64 + 1] operand image: 80 % 32 == 16 keeps k and k + 1 on disjoint banks
#define KF_SI 17            // LDS row stride of an [i][16] operand image

typedef float kf_f4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- explicit terms
// flux through the face half a cell from c0 towards cp, advecting velocity a, dh = delta / h
__device__ __forceinline__ float kf_flux(float a, float cm, float c0, float cp, float cpp, float dh) {
    const float C = a * dh;
    const float d = cp - c0;
    float low, high, num;
    if (a > 0.f) { low = c0; high = c0 + 0.5f * (1.f - C) * d; num = c0 - cm; }
    else { low = cp; high = cp - 0.5f * (1.f + C) * d; num = cpp - cp; }
    const float r = d != 0.f ? num / d : 0.f;
    const float ar = fabsf(r);
    const float phi = (r + ar) / (1.f + ar);
    return (low + phi * (high - low)) * a;
}

__global__ __launch_bounds__(KF_THREADS) void kflow_explicit_kernel(const float* __restrict__ x, int64_t x_sb, int n, float delta,
                                                                    float nu, float h, float dh, const float* __restrict__ forcing,
                                                                    float* __restrict__ out) {
    __shared__ float su[KF_LT][KF_LT + 1], sv[KF_LT][KF_LT + 1];
    const int i0 = blockIdx.y * KF_T, j0 = blockIdx.x * KF_T;
    const float* xb = x + (int64_t)blockIdx.z * x_sb;
    const int64_t plane = (int64_t)n * n;
    for (int e = threadIdx.x; e < KF_LT * KF_LT; e += KF_THREADS) {
        const int r = e / KF_LT, c = e - r * KF_LT;
        int gi = i0 + r - KF_HALO, gj = j0 + c - KF_HALO;
        gi = gi < 0 ? gi + n : (gi >= n ? gi - n : gi);
        gj = gj < 0 ? gj + n : (gj >= n ? gj - n : gj);
        su[r][c] = xb[(int64_t)gi * n + gj];
        sv[r][c] = xb[plane + (int64_t)gi * n + gj];
    }
    __syncthreads();
    const int li = (threadIdx.x >> 4) + KF_HALO, lj = (threadIdx.x & 15) + KF_HALO;
#define U(di, dj) su[li + (di)][lj + (dj)]
#define V(di, dj) sv[li + (di)][lj + (dj)]
    const float h2 = h * h;
    // u at ((i + 1) h, (j + 1/2) h)
    const float fx = kf_flux(0.5f * (U(0, 0) + U(1, 0)), U(-1, 0), U(0, 0), U(1, 0), U(2, 0), dh);
    const float fxm = kf_flux(0.5f * (U(-1, 0) + U(0, 0)), U(-2, 0), U(-1, 0), U(0, 0), U(1, 0), dh);
    const float fy = kf_flux(0.5f * (V(0, 0) + V(1, 0)), U(0, -1), U(0, 0), U(0, 1), U(0, 2), dh);
    const float fym = kf_flux(0.5f * (V(0, -1) + V(1, -1)), U(0, -2), U(0, -1), U(0, 0), U(0, 1), dh);
    const float adv_u = ((fx - fxm) + (fy - fym)) / h;
    const float lap_u = ((((U(1, 0) + U(-1, 0)) + U(0, 1)) + U(0, -1)) - 4.f * U(0, 0)) / h2;
    const int gj = j0 + lj - KF_HALO, gi = i0 + li - KF_HALO;
    const float f_u = forcing[gj] - 0.1f * U(0, 0);
    const float us = U(0, 0) + delta * ((nu * lap_u - adv_u) + f_u);
    // v at ((i + 1/2) h, (j + 1) h)
    const float gx = kf_flux(0.5f * (U(0, 0) + U(0, 1)), V(-1, 0), V(0, 0), V(1, 0), V(2, 0), dh);
    const float gxm = kf_flux(0.5f * (U(-1, 0) + U(-1, 1)), V(-2, 0), V(-1, 0), V(0, 0), V(1, 0), dh);
    const float gy = kf_flux(0.5f * (V(0, 0) + V(0, 1)), V(0, -1), V(0, 0), V(0, 1), V(0, 2), dh);
    const float gym = kf_flux(0.5f * (V(0, -1) + V(0, 0)), V(0, -2), V(0, -1), V(0, 0), V(0, 1), dh);
    const float adv_v = ((gx - gxm) + (gy - gym)) / h;
    const float lap_v = ((((V(1, 0) + V(-1, 0)) + V(0, 1)) + V(0, -1)) - 4.f * V(0, 0)) / h2;
    const float f_v = -0.1f * V(0, 0);
    const float vs = V(0, 0) + delta * ((nu * lap_v - adv_v) + f_v);
#undef U
#undef V
    float* ob = out + (int64_t)blockIdx.z * 2 * plane;
    ob[(int64_t)gi * n + gj] = us;
    ob[plane + (int64_t)gi * n + gj] = vs;
}

// ---------------------------------------------------------------- explicit terms, vector-Jacobian product
// w[0 .. 4] = lam x the partials of kf_flux with respect to (cm, c0, cp, cpp, a).  The conventions at the kinks are those of torch
// autograd on chains._kflow_flux: a > 0 selects the upwind branch (a == 0: the else branch) and a carries no derivative through the
// selection; d == 0 gives r = 0 with zero derivative; |r| has derivative sign(r), 0 at r == 0 (so phi'(0) = 1).
__device__ __forceinline__ void kf_flux_vjp(float a, float cm, float c0, float cp, float cpp, float dh, float lam, float* w) {
    const float C = a * dh;
    const float d = cp - c0;
    const bool pos = a > 0.f;
    const float low = pos ? c0 : cp;
    const float num = pos ? c0 - cm : cpp - cp;
    const float dhl = pos ? 0.5f * (1.f - C) : -0.5f * (1.f + C);    // d(high - low) / dd
    const float hl = dhl * d;                                         // high - low
    const bool nz = d != 0.f;
    const float id = nz ? 1.f / d : 0.f;
    const float r = nz ? num / d : 0.f;
    const float ar = fabsf(r);
    const float s = r > 0.f ? 1.f : (r < 0.f ? -1.f : 0.f);
    const float q1 = 1.f / (1.f + ar);
    const float phi = (r + ar) * q1;
    const float dphi = ((1.f + s) - phi * s) * q1;                    // d phi / dr
    const float gn = (hl * dphi) * id;                                // dQ / dnum, Q = low + phi (high - low)
    const float gd = phi * dhl - gn * r;                              // dQ / dd
    const float la = lam * a;
    w[0] = pos ? -la * gn : 0.f;
    w[1] = pos ? la * ((1.f + gn) - gd) : -la * gd;
    w[2] = pos ? la * gd : la * ((1.f + gd) - gn);
    w[3] = pos ? 0.f : la * gn;
    w[4] = lam * ((low + phi * hl) - a * (phi * (0.5f * dh * d)));
}

// gx = (dE/dx)^T g for E = kflow_explicit_kernel, linearised at x.  Phase A: every face the tile's cells touch gets its cotangent
// lam = -(delta / h) (g[i] - g[i + 1]) and lam x the five partials of its flux, into LDS.  Face kinds: 0 the x-faces of u, 1 the
// y-faces of u, 2 the x-faces of v, 3 the y-faces of v; x-faces are stored [KF_VFL][KF_VFC] (rows -2 .., columns -1 ..), y-faces
// [KF_VFC][KF_VFL] (rows -1 .., columns -2 ..).  Phase B: a cell is the cm, c0, cp, cpp tap of four faces along each axis of its own
// field, and enters the advecting velocity of two faces of each kind that averages its field -- a fixed-order sum per cell.
__global__ __launch_bounds__(KF_THREADS) void kflow_explicit_vjp_kernel(const float* __restrict__ x, int64_t x_sb,
                                                                        const float* __restrict__ g, int64_t g_sb, int n, float delta,
                                                                        float nu, float h, float dh, float* __restrict__ out) {
    constexpr int XS = KF_VLT + 1, GS = KF_VGT + 1;
    __shared__ float sx[2][KF_VLT * XS], sg[2][KF_VGT * GS];
    __shared__ float sw[4][5][KF_VFN];
    const int i0 = blockIdx.y * KF_T, j0 = blockIdx.x * KF_T;
    const float* xb = x + (int64_t)blockIdx.z * x_sb;
    const float* gb = g + (int64_t)blockIdx.z * g_sb;
    const int64_t plane = (int64_t)n * n;
    for (int e = threadIdx.x; e < KF_VLT * KF_VLT; e += KF_THREADS) {
        const int r = e / KF_VLT, c = e - r * KF_VLT;
        int gi = i0 + r - KF_VH, gj = j0 + c - KF_VH;
        gi = gi < 0 ? gi + n : (gi >= n ? gi - n : gi);
        gj = gj < 0 ? gj + n : (gj >= n ? gj - n : gj);
        sx[0][r * XS + c] = xb[(int64_t)gi * n + gj];
        sx[1][r * XS + c] = xb[plane + (int64_t)gi * n + gj];
    }
    for (int e = threadIdx.x; e < KF_VGT * KF_VGT; e += KF_THREADS) {
        const int r = e / KF_VGT, c = e - r * KF_VGT;
        int gi = i0 + r - KF_VG, gj = j0 + c - KF_VG;
        gi = gi < 0 ? gi + n : (gi >= n ? gi - n : gi);
        gj = gj < 0 ? gj + n : (gj >= n ? gj - n : gj);
        sg[0][r * GS + c] = gb[(int64_t)gi * n + gj];
        sg[1][r * GS + c] = gb[plane + (int64_t)gi * n + gj];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 4 * KF_VFN; e += KF_THREADS) {
        const int t = e / KF_VFN, f = e - t * KF_VFN;
        const bool xdir = !(t & 1);
        const int q = xdir ? f / KF_VFC : f / KF_VFL;
        const int r = xdir ? q - 2 : q - 1;
        const int c = xdir ? f - q * KF_VFC - 1 : f - q * KF_VFL - 2;
        const float* sc = sx[t >> 1];                     // the advected field
        const float* sa = sx[t & 1];                      // the field the advecting velocity averages ...
        const int at = (r + KF_VH) * XS + c + KF_VH;
        const int st = xdir ? XS : 1;
        const int ast = (t >> 1) ? 1 : XS;                // ... towards the neighbour in the direction the field is staggered
        const float* gg = sg[t >> 1];
        const int gat = (r + KF_VG) * GS + c + KF_VG;
        const float lam = -dh * (gg[gat] - gg[gat + (xdir ? GS : 1)]);
        float w[5];
        kf_flux_vjp(0.5f * (sa[at] + sa[at + ast]), sc[at - st], sc[at], sc[at + st], sc[at + 2 * st], dh, lam, w);
#pragma unroll
        for (int k = 0; k < 5; ++k) sw[t][k][f] = w[k];
    }
    __syncthreads();
    const int li = threadIdx.x >> 4, lj = threadIdx.x & 15;
#define FX(t, k, di, dj) sw[t][k][(li + (di) + 2) * KF_VFC + lj + (dj) + 1]
#define FY(t, k, di, dj) sw[t][k][(li + (di) + 1) * KF_VFL + lj + (dj) + 2]
#define G(p, di, dj) sg[p][(li + (di) + KF_VG) * GS + lj + (dj) + KF_VG]
    const float h2 = h * h;
    // the diffusion, drag and identity terms are linear and symmetric: their adjoint is the same stencil on g
    const float lap_u = ((((G(0, 1, 0) + G(0, -1, 0)) + G(0, 0, 1)) + G(0, 0, -1)) - 4.f * G(0, 0, 0)) / h2;
    const float lap_v = ((((G(1, 1, 0) + G(1, -1, 0)) + G(1, 0, 1)) + G(1, 0, -1)) - 4.f * G(1, 0, 0)) / h2;
    float gu = G(0, 0, 0) + delta * (nu * lap_u - 0.1f * G(0, 0, 0));
    float gv = G(1, 0, 0) + delta * (nu * lap_v - 0.1f * G(1, 0, 0));
    gu += (FX(0, 0, 1, 0) + FX(0, 1, 0, 0)) + (FX(0, 2, -1, 0) + FX(0, 3, -2, 0));
    gu += (FY(1, 0, 0, 1) + FY(1, 1, 0, 0)) + (FY(1, 2, 0, -1) + FY(1, 3, 0, -2));
    gu += 0.5f * ((FX(0, 4, 0, 0) + FX(0, 4, -1, 0)) + (FX(2, 4, 0, 0) + FX(2, 4, 0, -1)));
    gv += (FX(2, 0, 1, 0) + FX(2, 1, 0, 0)) + (FX(2, 2, -1, 0) + FX(2, 3, -2, 0));
    gv += (FY(3, 0, 0, 1) + FY(3, 1, 0, 0)) + (FY(3, 2, 0, -1) + FY(3, 3, 0, -2));
    gv += 0.5f * ((FY(1, 4, 0, 0) + FY(1, 4, -1, 0)) + (FY(3, 4, 0, 0) + FY(3, 4, 0, -1)));
#undef FX
#undef FY
#undef G
    float* ob = out + (int64_t)blockIdx.z * 2 * plane;
    const int64_t at = (int64_t)(i0 + li) * n + j0 + lj;
    ob[at] = gu;
    ob[plane + at] = gv;
}

// ---------------------------------------------------------------- dense products with Hm
struct KfGemm {
    const float* x;         // SIDE 0: the B operand [n][n] (VAR 1: the velocity pair the divergence is taken of); SIDE 1: the A operand
    int64_t x_sb;
    const float* hm;
    const float* scale;     // SIDE 1, VAR 0: optional [n][n] factor on the result
    const float* uv;        // SIDE 1, VAR 1: the velocity pair the gradient is subtracted from
    int64_t uv_sb;
    float* out;
    int64_t out_sb;
    int n;
    float h;
};

__device__ __forceinline__ int kf_wrap(int i, int n) { return i % n; }

// SIDE 0: out = Hm X (VAR 1: X = div(u, v)).  SIDE 1: out = (X Hm) o scale (VAR 1: out = uv - grad(X Hm)).
// 64 x 64 tile per workgroup, wave w owns the 32 x 32 quadrant (w >> 1, w & 1) as 2 x 2 fragments.  Rows and columns past n wrap
// (n % 16 == 0: a fragment is wholly inside or wholly outside, and only inside ones are stored).
template <int SIDE, int VAR>
__global__ __launch_bounds__(KF_THREADS) void kflow_gemm_kernel(KfGemm g) {
    constexpr bool GRAD = SIDE == 1 && VAR == 1;
    constexpr int A_SI = SIDE == 0 ? 1 : KF_SI, A_SK = SIDE == 0 ? KF_SK : 1;
    constexpr int A_FLOATS = SIDE == 0 ? KF_KC * KF_SK : (KF_TILE + 1) * KF_SI;
    __shared__ float As[A_FLOATS], Bs[KF_KC * KF_SK];
    const int n = g.n, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int i0 = blockIdx.y * KF_TILE, j0 = blockIdx.x * KF_TILE;
    const float* xb = g.x + (int64_t)blockIdx.z * g.x_sb;
    const int64_t plane = (int64_t)n * n;

    // staging registers: 4 floats of A and 4 of B per thread, plus the extra row / column of the gradient form
    kf_f4 ra, rb;
    float ea = 0.f, eb = 0.f;
    const int kr = t >> 4, c4 = (t & 15) * 4;             // [k][64] images: row k, columns c4 .. c4 + 3
    const int ar = t >> 2, ak4 = (t & 3) * 4;             // [i][16] image: row i, k = ak4 .. ak4 + 3
    // the wrapped row / column a thread loads from does not depend on the k-chunk: resolved once, outside the k loop
    const int wa = kf_wrap(i0 + (SIDE == 0 ? c4 : ar), n), wb = kf_wrap(j0 + c4, n);
    const int wea = kf_wrap(i0 + KF_TILE, n), web = kf_wrap(j0 + KF_TILE, n);
    const float* pa = SIDE == 0 ? g.hm + (int64_t)kr * n + wa : xb + (int64_t)wa * n + ak4;      // Hm is symmetric: A[i][k] = Hm[k][i]
    const float* pb = SIDE == 0 ? xb + wb : g.hm + (int64_t)kr * n + wb;
    const int wbl = wb == 0 ? n - 1 : wb - 1;
    const int te = t < KF_KC ? t : 0;                     // only the first KF_KC threads load the extra row / column
    const float* pea = xb + (int64_t)wea * n + te;
    const float* peb = g.hm + (int64_t)te * n + web;
    auto fetch = [&](int k0) {
        if (SIDE == 0) {
            ra = *(const kf_f4*)(pa + (int64_t)k0 * n);
            const int row = k0 + kr;
            if (VAR == 0) {
                rb = *(const kf_f4*)(pb + (int64_t)row * n);
            } else {
                const int rm = row == 0 ? n - 1 : row - 1;
                const kf_f4 u0 = *(const kf_f4*)(pb + (int64_t)row * n), um = *(const kf_f4*)(pb + (int64_t)rm * n);
                const kf_f4 v0 = *(const kf_f4*)(pb + plane + (int64_t)row * n);
                const float vl = xb[plane + (int64_t)row * n + wbl];
                rb.x = ((u0.x - um.x) + (v0.x - vl)) / g.h;
                rb.y = ((u0.y - um.y) + (v0.y - v0.x)) / g.h;
                rb.z = ((u0.z - um.z) + (v0.z - v0.y)) / g.h;
                rb.w = ((u0.w - um.w) + (v0.w - v0.z)) / g.h;
            }
        } else {
            ra = *(const kf_f4*)(pa + k0);
            rb = *(const kf_f4*)(pb + (int64_t)k0 * n);
            if (GRAD) {
                if (t < KF_KC) {
                    ea = pea[k0];
                    eb = peb[(int64_t)k0 * n];
                }
            }
        }
    };
    auto stage = [&]() {
        if (SIDE == 0) {
            float* a = As + kr * KF_SK + c4;
            a[0] = ra.x; a[1] = ra.y; a[2] = ra.z; a[3] = ra.w;
        } else {
            float* a = As + ar * KF_SI + ak4;
            a[0] = ra.x; a[1] = ra.y; a[2] = ra.z; a[3] = ra.w;
            if (GRAD && t < KF_KC) { As[KF_TILE * KF_SI + t] = ea; Bs[t * KF_SK + KF_TILE] = eb; }
        }
        float* b = Bs + kr * KF_SK + c4;
        b[0] = rb.x; b[1] = rb.y; b[2] = rb.z; b[3] = rb.w;
    };

    kf_f4 acc[2][2], accx[2][2], accy[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[m][q] = accx[m][q] = accy[m][q] = kf_f4{0.f, 0.f, 0.f, 0.f};
    const int ib = 32 * (w >> 1), jb = 32 * (w & 1);
    const int fl = lane & 15, fk = lane >> 4;

    fetch(0);
    for (int k0 = 0; k0 < n; k0 += KF_KC) {
        __syncthreads();                                  // the previous chunk's reads are done
        stage();
        __syncthreads();
        if (k0 + KF_KC < n) fetch(k0 + KF_KC);            // in flight under the multiply
        // blocked summation: each chunk of 16 k starts from zero and joins the running sum once, so a sum over n terms rounds like
        // one over 16 + n / 16 (a single 256-term fma chain is ~3x less accurate than the FFT it is checked against)
        kf_f4 c[2][2], cx[2][2], cy[2][2];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int q = 0; q < 2; ++q) c[m][q] = cx[m][q] = cy[m][q] = kf_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < KF_KC / 4; ++kk) {
            const int k = 4 * kk + fk;
            float a[2], b[2], ax[2], by[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                a[m] = As[(ib + 16 * m + fl) * A_SI + k * A_SK];
                b[m] = Bs[k * KF_SK + jb + 16 * m + fl];
                if (GRAD) {
                    ax[m] = As[(ib + 16 * m + fl + 1) * A_SI + k * A_SK];
                    by[m] = Bs[k * KF_SK + jb + 16 * m + fl + 1];
                }
            }
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    c[m][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], b[q], c[m][q], 0, 0, 0);
                    if (GRAD) {
                        cx[m][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(ax[m], b[q], cx[m][q], 0, 0, 0);
                        cy[m][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], by[q], cy[m][q], 0, 0, 0);
                    }
                }
        }
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                acc[m][q] += c[m][q];
                if (GRAD) { accx[m][q] += cx[m][q]; accy[m][q] += cy[m][q]; }
            }
    }

    // D fragment: column = lane & 15, row = 4 (lane >> 4) + r
    float* ob = g.out + (int64_t)blockIdx.z * g.out_sb;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int fi = i0 + ib + 16 * m, fj = j0 + jb + 16 * q;
            if (fi >= n || fj >= n) continue;             // wave-uniform
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t at = (int64_t)(fi + 4 * fk + r) * n + fj + fl;
                const float v = acc[m][q][r];
                if (GRAD) {
                    const float* uvb = g.uv + (int64_t)blockIdx.z * g.uv_sb;
                    ob[at] = uvb[at] - (accx[m][q][r] - v) / g.h;
                    ob[plane + at] = uvb[plane + at] - (accy[m][q][r] - v) / g.h;
                } else if (SIDE == 1 && g.scale) {
                    ob[at] = v * g.scale[at];
                } else {
                    ob[at] = v;
                }
            }
        }
}

// ---------------------------------------------------------------- host side
static inline float kf_h(int n) { return (float)(6.283185307179586476925286766559 / (double)n); }

extern "C" int sda_kflow_serves(int n) { return n >= 16 && n <= 512 && n % 16 == 0; }

extern "C" int64_t sda_kflow_work_floats(int n, int nb) {
    if (!sda_kflow_serves(n) || nb < 1) return 0;
    return 6 * (int64_t)nb * n * n;                       // u*, v* | T a | T b | the running state
}

static int kf_model_check(const sda_kflow_model* m, int nb) {
    if (!m || !m->hm || !m->inv || !m->forcing || nb < 1 || m->steps < 1 || !(m->delta > 0.f) || !(m->nu >= 0.f)) return SDA_E_BADARG;
    if (!sda_kflow_serves(m->n) || nb > 65535) return SDA_E_UNSUPPORTED;
    return SDA_OK;
}

static inline dim3 kf_gemm_grid(int n, int nb) {
    const unsigned tiles = (unsigned)((n + KF_TILE - 1) / KF_TILE);
    return dim3(tiles, tiles, (unsigned)nb);
}

static void kf_launch_explicit(const sda_kflow_model* m, const float* x, int64_t x_sb, int nb, float* out, hipStream_t st) {
    const float h = kf_h(m->n);
    const float dh = (float)((double)m->delta / (6.283185307179586476925286766559 / (double)m->n));
    hipLaunchKernelGGL(kflow_explicit_kernel, dim3(m->n / KF_T, m->n / KF_T, nb), dim3(KF_THREADS), 0, st, x, x_sb, m->n, m->delta,
                       m->nu, h, dh, m->forcing, out);
}

static void kf_launch_explicit_vjp(const sda_kflow_model* m, const float* x, int64_t x_sb, const float* g, int64_t g_sb, int nb, float* out,
                                   hipStream_t st) {
    const float h = kf_h(m->n);
    const float dh = (float)((double)m->delta / (6.283185307179586476925286766559 / (double)m->n));
    hipLaunchKernelGGL(kflow_explicit_vjp_kernel, dim3(m->n / KF_T, m->n / KF_T, nb), dim3(KF_THREADS), 0, st, x, x_sb, g, g_sb, m->n,
                       m->delta, m->nu, h, dh, out);
}

// out = uv - grad(lap^-1 div(uv)): four launches; ta, tb: nb planes each
static void kf_launch_project(const sda_kflow_model* m, const float* uv, int64_t uv_sb, int nb, float* out, int64_t out_sb, float* ta,
                              float* tb, hipStream_t st) {
    const int n = m->n;
    const int64_t plane = (int64_t)n * n;
    const dim3 grid = kf_gemm_grid(n, nb);
    KfGemm g;
    g.hm = m->hm; g.n = n; g.h = kf_h(n); g.scale = nullptr; g.uv = nullptr; g.uv_sb = 0;
    g.x = uv; g.x_sb = uv_sb; g.out = ta; g.out_sb = plane;
    hipLaunchKernelGGL((kflow_gemm_kernel<0, 1>), grid, dim3(KF_THREADS), 0, st, g);
    g.x = ta; g.x_sb = plane; g.out = tb; g.scale = m->inv;
    hipLaunchKernelGGL((kflow_gemm_kernel<1, 0>), grid, dim3(KF_THREADS), 0, st, g);
    g.x = tb; g.out = ta; g.scale = nullptr;
    hipLaunchKernelGGL((kflow_gemm_kernel<0, 0>), grid, dim3(KF_THREADS), 0, st, g);
    g.x = ta; g.uv = uv; g.uv_sb = uv_sb; g.out = out; g.out_sb = out_sb;
    hipLaunchKernelGGL((kflow_gemm_kernel<1, 1>), grid, dim3(KF_THREADS), 0, st, g);
}

extern "C" int sda_kflow_explicit(const sda_kflow_model* m, const float* x, int64_t x_sb, int nb, float* out, void* stream) {
    int rc = kf_model_check(m, nb);
    if (rc != SDA_OK) return rc;
    if (!x || !out || x_sb < 2 * (int64_t)m->n * m->n) return SDA_E_BADARG;
    kf_launch_explicit(m, x, x_sb, nb, out, (hipStream_t)stream);
    return sda_launch_status();
}

extern "C" int sda_kflow_hartley(const float* hm, int n, const float* x, int64_t x_sb, int nb, int side, const float* scale, float* out,
                                 void* stream) {
    if (!hm || !x || !out || nb < 1 || (side != 0 && side != 1) || (side == 0 && scale) || x == out) return SDA_E_BADARG;
    if (!sda_kflow_serves(n) || nb > 65535) return SDA_E_UNSUPPORTED;
    if (x_sb < (int64_t)n * n || x_sb % 4 != 0) return SDA_E_BADARG;
    KfGemm g;
    g.hm = hm; g.n = n; g.h = kf_h(n); g.scale = scale; g.uv = nullptr; g.uv_sb = 0;
    g.x = x; g.x_sb = x_sb; g.out = out; g.out_sb = (int64_t)n * n;
    if (side == 0) hipLaunchKernelGGL((kflow_gemm_kernel<0, 0>), kf_gemm_grid(n, nb), dim3(KF_THREADS), 0, (hipStream_t)stream, g);
    else hipLaunchKernelGGL((kflow_gemm_kernel<1, 0>), kf_gemm_grid(n, nb), dim3(KF_THREADS), 0, (hipStream_t)stream, g);
    return sda_launch_status();
}

extern "C" int sda_kflow_project(const sda_kflow_model* m, const float* x, int64_t x_sb, int nb, float* out, int64_t out_sb, float* work,
                                 void* stream) {
    int rc = kf_model_check(m, nb);
    if (rc != SDA_OK) return rc;
    const int64_t plane = (int64_t)m->n * m->n;
    if (!x || !out || !work || x_sb < 2 * plane || out_sb < 2 * plane || x_sb % 4 != 0) return SDA_E_BADARG;
    kf_launch_project(m, x, x_sb, nb, out, out_sb, work, work + nb * plane, (hipStream_t)stream);
    return sda_launch_status();
}

extern "C" int sda_kflow_advance(const sda_kflow_model* m, const float* x, int64_t x_sb, int nb, int transitions, int every, float* out,
                                 int64_t out_st, float* work, void* stream) {
    int rc = kf_model_check(m, nb);
    if (rc != SDA_OK) return rc;
    const int64_t plane = (int64_t)m->n * m->n;
    if (!x || !out || !work || transitions < 1 || x_sb < 2 * plane || (every && out_st < 2 * plane * nb)) return SDA_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    float* ustar = work;
    float* ta = work + 2 * nb * plane;
    float* tb = ta + nb * plane;
    float* state = tb + nb * plane;
    const float* cur = x;
    int64_t cur_sb = x_sb;
    for (int t = 0; t < transitions; ++t)
        for (int s = 0; s < m->steps; ++s) {
            // the state a transition ends in goes straight to where the caller keeps it
            const bool keep = s == m->steps - 1 && (every || t == transitions - 1);
            float* dst = keep ? out + (every ? t * out_st : 0) : state;
            kf_launch_explicit(m, cur, cur_sb, nb, ustar, st);
            kf_launch_project(m, ustar, 2 * plane, nb, dst, 2 * plane, ta, tb, st);
            cur = dst;
            cur_sb = 2 * plane;
            rc = sda_launch_status();
            if (rc != SDA_OK) return rc;
        }
    return SDA_OK;
}

// ---------------------------------------------------------------- the adjoint of a transition
extern "C" int64_t sda_kfvjp_work_floats(int n, int nb, int steps) {
    if (!sda_kflow_serves(n) || nb < 1 || steps < 1) return 0;
    // the states sub-steps 1 .. steps - 1 start from | u* of the recompute, then P g | T a, T b | the running cotangent
    return ((int64_t)steps + 2) * 2 * nb * n * n;
}

extern "C" int sda_kfvjp_explicit(const sda_kflow_model* m, const float* x, int64_t x_sb, const float* g, int64_t g_sb, int nb, float* out,
                                  void* stream) {
    int rc = kf_model_check(m, nb);
    if (rc != SDA_OK) return rc;
    const int64_t plane = (int64_t)m->n * m->n;
    if (!x || !g || !out || x_sb < 2 * plane || g_sb < 2 * plane || out == x || out == g) return SDA_E_BADARG;
    kf_launch_explicit_vjp(m, x, x_sb, g, g_sb, nb, out, (hipStream_t)stream);
    return sda_launch_status();
}

extern "C" int sda_kfvjp_transition(const sda_kflow_model* m, const float* x0, int64_t x0_sb, const float* g, int64_t g_sb, int nb,
                                    float* out, float* work, void* stream) {
    int rc = kf_model_check(m, nb);
    if (rc != SDA_OK) return rc;
    const int64_t plane = (int64_t)m->n * m->n, field = 2 * plane, slab = field * nb;
    if (!x0 || !g || !out || !work || x0_sb < field || g_sb < field || g_sb % 4 != 0 || out == x0) return SDA_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int steps = m->steps;
    float* states = work;                                 // states[s - 1]: what sub-step s starts from, s = 1 .. steps - 1
    float* tmp = work + (int64_t)(steps - 1) * slab;
    float* ta = tmp + slab;
    float* tb = ta + nb * plane;
    float* run = ta + slab;
    // forward again, with the launches of sda_kflow_advance: bitwise the states the forward pass went through
    const float* cur = x0;
    int64_t cur_sb = x0_sb;
    for (int s = 0; s + 1 < steps; ++s) {
        float* dst = states + (int64_t)s * slab;
        kf_launch_explicit(m, cur, cur_sb, nb, tmp, st);
        kf_launch_project(m, tmp, field, nb, dst, field, ta, tb, st);
        cur = dst;
        cur_sb = field;
        rc = sda_launch_status();
        if (rc != SDA_OK) return rc;
    }
    // backwards: g <- P g (P is its own transpose), then g <- E'(x_s)^T g
    const float* gc = g;
    int64_t gc_sb = g_sb;
    for (int s = steps - 1; s >= 0; --s) {
        const float* xs = s ? states + (int64_t)(s - 1) * slab : x0;
        float* dst = s ? run : out;
        kf_launch_project(m, gc, gc_sb, nb, tmp, field, ta, tb, st);
        kf_launch_explicit_vjp(m, xs, s ? field : x0_sb, tmp, field, nb, dst, st);
        gc = dst;
        gc_sb = field;
        rc = sda_launch_status();
        if (rc != SDA_OK) return rc;
    }
    return SDA_OK;
}
