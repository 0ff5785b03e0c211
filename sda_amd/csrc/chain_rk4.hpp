// The RK4 transition of the Markov chains (sda/mcs.py:98-110) and its reverse sweep, written ONCE over a "system" policy, and the
// four systems chain.hip runs it on.  A system has
//   N                    capacity of the per-thread component array (compile time)
//   n()                  live components (constexpr except for the array form of Lorenz-96)
//   Keep                 what f leaves for the Jacobian at the same stage point
//   f(v, k, keep)        k = f(v)
//   jt(v, keep, gk, o)   o = J_f(v)^T gk
// Every object is compiled with -ffp-contract=off and every form goes through the same scalar helpers in the same order, so the
// device kernels and the host replay (SDA_HOST_EMU) run the same stage sequence: only the Lorenz-96 neighbour access differs
// (shuffles on the device, array indices on the host), and both take their neighbours from l96_lanes.
#pragma once
#include "sda_common.hpp"

// ---------------------------------------------------------------- one component, reference order
__host__ __device__ __forceinline__ float rk4_half(float x, float h, float k) { return x + h * k / 2.0f; }
__host__ __device__ __forceinline__ float rk4_full(float x, float h, float k) { return x + h * k; }
__host__ __device__ __forceinline__ float rk4_comb(float x, float h, float k1, float k2, float k3, float k4) {
    return x + h * (k1 + 2.0f * k2 + 2.0f * k3 + k4) / 6.0f;
}
// the reverse sweep of one sub-step.  With gy the cotangent of y = x + h (k1 + 2 k2 + 2 k3 + k4) / 6 and jt_i = J_f(v_i)^T gk_i at
// the recomputed stage point v_i (v_1 = x):
//   gk4 = h/6 gy, gk3 = h/3 gy + h jt4, gk2 = h/3 gy + h/2 jt3, gk1 = h/6 gy + h/2 jt2, gx = gy + jt4 + jt3 + jt2 + jt1.
__host__ __device__ __forceinline__ float rk4r_k4(float h, float gy) { return h * gy / 6.0f; }
__host__ __device__ __forceinline__ float rk4r_k3(float h, float gy, float jt4) { return h * gy / 3.0f + h * jt4; }
__host__ __device__ __forceinline__ float rk4r_k2(float h, float gy, float jt3) { return h * gy / 3.0f + h * jt3 / 2.0f; }
__host__ __device__ __forceinline__ float rk4r_k1(float h, float gy, float jt2) { return h * gy / 6.0f + h * jt2 / 2.0f; }
__host__ __device__ __forceinline__ float rk4r_x(float gy, float jt1, float jt2, float jt3, float jt4) { return gy + jt4 + jt3 + jt2 + jt1; }

// ---------------------------------------------------------------- the stage sequence
// x <- one RK4 sub-step from x
template <class Sys>
__host__ __device__ __forceinline__ void rk4_substep(const Sys& sys, float h, float* x) {
    constexpr int N = Sys::N;
    const int n = sys.n();
    float k1[N], k2[N], k3[N], k4[N], t[N];
    typename Sys::Keep keep;
    sys.f(x, k1, keep);
    for (int c = 0; c < n; ++c) t[c] = rk4_half(x[c], h, k1[c]);
    sys.f(t, k2, keep);
    for (int c = 0; c < n; ++c) t[c] = rk4_half(x[c], h, k2[c]);
    sys.f(t, k3, keep);
    for (int c = 0; c < n; ++c) t[c] = rk4_full(x[c], h, k3[c]);
    sys.f(t, k4, keep);
    for (int c = 0; c < n; ++c) x[c] = rk4_comb(x[c], h, k1[c], k2[c], k3[c], k4[c]);
}

// one transition: `steps` sub-steps
template <class Sys>
__host__ __device__ __forceinline__ void rk4_transition(const Sys& sys, float h, int steps, float* x) {
    for (int s = 0; s < steps; ++s) rk4_substep(sys, h, x);
}

// g <- (d sub-step / dx at x)^T g: the four stage points recomputed, then j4 -> j3 -> j2 -> j1
template <class Sys>
__host__ __device__ __forceinline__ void rk4_substep_vjp(const Sys& sys, float h, const float* x, float* g) {
    constexpr int N = Sys::N;
    const int n = sys.n();
    float k[N], v2[N], v3[N], v4[N], gk[N], j1[N], j2[N], j3[N], j4[N];
    typename Sys::Keep e1, e2, e3, e4;
    sys.f(x, k, e1);
    for (int c = 0; c < n; ++c) v2[c] = rk4_half(x[c], h, k[c]);
    sys.f(v2, k, e2);
    for (int c = 0; c < n; ++c) v3[c] = rk4_half(x[c], h, k[c]);
    sys.f(v3, k, e3);
    for (int c = 0; c < n; ++c) v4[c] = rk4_full(x[c], h, k[c]);
    sys.f(v4, k, e4);                                   // (only e4 is used: k4 itself does not enter the reverse sweep)
    for (int c = 0; c < n; ++c) gk[c] = rk4r_k4(h, g[c]);
    sys.jt(v4, e4, gk, j4);
    for (int c = 0; c < n; ++c) gk[c] = rk4r_k3(h, g[c], j4[c]);
    sys.jt(v3, e3, gk, j3);
    for (int c = 0; c < n; ++c) gk[c] = rk4r_k2(h, g[c], j3[c]);
    sys.jt(v2, e2, gk, j2);
    for (int c = 0; c < n; ++c) gk[c] = rk4r_k1(h, g[c], j2[c]);
    sys.jt(x, e1, gk, j1);
    for (int c = 0; c < n; ++c) g[c] = rk4r_x(g[c], j1[c], j2[c], j3[c], j4[c]);
}

// g <- (d transition / dx at x0)^T g.  The states inside a transition are not stored: sub-step s, last to first, starts from x0
// advanced s sub-steps again (O(steps^2) on n floats, bitwise the forward's states).
template <class Sys>
__host__ __device__ __forceinline__ void rk4_transition_vjp(const Sys& sys, float h, int steps, const float* x0, float* g) {
    const int n = sys.n();
    for (int s = steps - 1; s >= 0; --s) {
        float x[Sys::N];
        for (int c = 0; c < n; ++c) x[c] = x0[c];
        rk4_transition(sys, h, s, x);
        rk4_substep_vjp(sys, h, x, g);
    }
}

// ---------------------------------------------------------------- the systems
struct KeepNothing {};

// sda/mcs.py:153-158; p = (sigma, rho, beta)
struct Lorenz63Sys {
    static constexpr int N = 3;
    typedef KeepNothing Keep;
    const float* p;
    __host__ __device__ static constexpr int n() { return N; }
    __host__ __device__ __forceinline__ void f(const float* x, float* k, Keep&) const {
        k[0] = p[0] * (x[1] - x[0]);
        k[1] = x[0] * (p[1] - x[2]) - x[1];
        k[2] = x[0] * x[1] - p[2] * x[2];
    }
    __host__ __device__ __forceinline__ void jt(const float* v, const Keep&, const float* g, float* o) const {
        o[0] = (p[1] - v[2]) * g[1] - p[0] * g[0] + v[1] * g[2];
        o[1] = p[0] * g[0] - g[1] + v[0] * g[2];
        o[2] = -(v[0] * g[1]) - p[2] * g[2];
    }
};

// sda/mcs.py:237-241; p = (alpha, beta, delta, gamma).  f keeps e = exp of the stage point: the Jacobian needs the same two expf
struct LotkaVolterraSys {
    static constexpr int N = 2;
    struct Keep { float e[2]; };
    const float* p;
    __host__ __device__ static constexpr int n() { return N; }
    __host__ __device__ __forceinline__ void f(const float* x, float* k, Keep& a) const {
        a.e[0] = expf(x[0]);
        a.e[1] = expf(x[1]);
        k[0] = p[0] - p[1] * a.e[1];
        k[1] = p[2] * a.e[0] - p[3];
    }
    __host__ __device__ __forceinline__ void jt(const float*, const Keep& a, const float* g, float* o) const {
        o[0] = p[2] * a.e[0] * g[1];
        o[1] = -(p[1] * a.e[1] * g[0]);
    }
};

// sda/mcs.py:208-211: (roll(x, 1) - roll(x, -2)) roll(x, -1) - x + F, one component
__host__ __device__ __forceinline__ float lorenz96_f(float xm1, float xp2, float xp1, float x, float F) {
    return (xm1 - xp2) * xp1 - x + F;
}
// in gather form: f_c = (x_{c-1} - x_{c+2}) x_{c+1} - x_c + F reaches x_j from c = j + 1, j - 2 and j - 1 (and j itself)
__host__ __device__ __forceinline__ float lorenz96_jt(float gp1, float xp2, float gm2, float xm1, float gm1, float xm2, float xp1,
                                                      float g) {
    return gp1 * xp2 - gm2 * xm1 + gm1 * (xm2 - xp1) - g;
}
// where components c - 1, c + 1, c + 2 and c - 2 (modulo n) of a particle live, counted from `base`: roll(x, 1)[c] = x[c - 1],
// roll(x, -1)[c] = x[c + 1], roll(x, -2)[c] = x[c + 2].  Lanes of the wave on the device, array indices (base = 0) on the host.
struct L96Lanes { int m1, p1, p2, m2; };
__host__ __device__ __forceinline__ L96Lanes l96_lanes(int base, int c, int n) {
    return {base + (c + n - 1) % n, base + (c + 1) % n, base + (c + 2) % n, base + (c + n - 2) % n};
}

#ifndef SDA_HOST_EMU
// Lorenz-96 on lanes: this lane's component, its neighbours by shuffle.  EVERY lane of the wave calls f and jt (dead lanes carry
// zeros); only the caller's loads and stores are predicated.
struct L96LaneSys {
    static constexpr int N = 1;
    struct Keep { float m1, p1, p2; };      // a stage point's values at c - 1, c + 1, c + 2
    L96Lanes l;
    float F;
    __device__ static constexpr int n() { return N; }
    __device__ __forceinline__ void f(const float* v, float* k, Keep& a) const {
        a = {__shfl(v[0], l.m1, SDA_WAVE), __shfl(v[0], l.p1, SDA_WAVE), __shfl(v[0], l.p2, SDA_WAVE)};
        k[0] = lorenz96_f(a.m1, a.p2, a.p1, v[0], F);
    }
    // the stage point's three forward shuffles are reused, v_{c-2} and three of gk are the four new ones
    __device__ __forceinline__ void jt(const float* v, const Keep& a, const float* gk, float* o) const {
        o[0] = lorenz96_jt(__shfl(gk[0], l.p1, SDA_WAVE), a.p2, __shfl(gk[0], l.m2, SDA_WAVE), a.m1, __shfl(gk[0], l.m1, SDA_WAVE),
                           __shfl(v[0], l.m2, SDA_WAVE), a.p1, gk[0]);
    }
};
#else
// Lorenz-96 with a particle in one array (host replay only)
struct L96ArraySys {
    static constexpr int N = 64;
    typedef KeepNothing Keep;
    int d;
    float F;
    int n() const { return d; }
    void f(const float* v, float* k, Keep&) const {
        for (int c = 0; c < d; ++c) {
            const L96Lanes l = l96_lanes(0, c, d);
            k[c] = lorenz96_f(v[l.m1], v[l.p2], v[l.p1], v[c], F);
        }
    }
    void jt(const float* v, const Keep&, const float* gk, float* o) const {
        for (int c = 0; c < d; ++c) {
            const L96Lanes l = l96_lanes(0, c, d);
            o[c] = lorenz96_jt(gk[l.p1], v[l.p2], gk[l.m2], v[l.m1], gk[l.m1], v[l.m2], v[l.p1], gk[c]);
        }
    }
};
#endif
