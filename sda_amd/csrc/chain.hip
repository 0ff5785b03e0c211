// Markov chains (sda/mcs.py:85-241) and the bootstrap particle filter (sda/utils.py:168-200) of the reference's Lorenz
// evaluation (experiments/lorenz/eval.py:44-68), as one launch per PHASE: advance (+ log-weights) -> cdf -> resample per
// observation, one traceback at the end.  No kernel waits for another workgroup: every hand-off is a launch boundary.
// The arithmetic of a transition is not mirrored between device and host: it IS one piece of code.  The RK4 stage sequence, its
// reverse sweep and the recompute loop are templates over a system policy (chain_rk4.hpp), and the noise, log-density, resampling
// and traceback are __host__ __device__ functions here; under SDA_HOST_EMU the same functions run inside plain loops over host
// arrays (bottom of the file), which is what the CPU tests check.  Shared: every float operation and its order.  Not shared: the
// kernels' geometry and wave reductions, and how Lorenz-96 reaches a neighbour component -- a shuffle on the device (L96LaneSys),
// an array index on the host (L96ArraySys), both wired by l96_lanes.
//
// Latency-bound by design: 16 384 particles x 3 floats is 192 KiB, one RK4 transition is ~100 flops per particle.  What the
// fusion removes is the ~40 elementwise launches per transition and the O(M T^2) history copies of the reference's
// cat / x[j] (sda/utils.py:193-200).
#include "sda_common.hpp"
#include "chain_check.hpp"
#include "chain_rk4.hpp"
#include "philox.hpp"

#define CH_THREADS 256

// the system of a small-state model kind (one particle in the registers of one lane)
template <int KIND> struct ChainSmall { typedef Lorenz63Sys Sys; };
template <> struct ChainSmall<SDA_CHAIN_LOTKA_VOLTERRA> { typedef LotkaVolterraSys Sys; };

// the four normals of quad q of global row `grow` in draw t of the sda_randn_rows stream
__host__ __device__ __forceinline__ void chain_noise4(uint64_t seed, uint64_t grow, int64_t t, int64_t q, float* z) {
    philox_normal4(q, grow, t, (uint32_t)seed, (uint32_t)(seed >> 32), z);
}

// log N(v; mu, s) as torch.distributions.Normal.log_prob writes it, in float64
__host__ __device__ __forceinline__ double normal_log_prob(double v, double mu, double s) {
    const double d = v - mu;
    return -(d * d) / (2.0 * s * s) - log(s) - 0.91893853320467274178;
}

// the affine-select log-weight of one state (y: the k observed values)
__host__ __device__ __forceinline__ float obs_logweight(const sda_chain_obs& o, const float* y, const float* x) {
    double l = 0.0;
    for (int k = 0; k < o.k; ++k) l += normal_log_prob((double)((x[o.idx[k]] - o.shift[k]) / o.scale[k]), (double)y[k], (double)o.sigma);
    return (float)l;
}

// u in (0, 1): 52 Philox bits and a set 53rd, exact in float64
__host__ __device__ __forceinline__ double bpf_uniform(uint64_t seed, int64_t j, int64_t obs) {
    const philox4 w = philox4x32_10((uint32_t)j, (uint32_t)obs, 0x80000000u | (uint32_t)((uint64_t)j >> 32), 0x52455341u,
                                    (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint64_t v = ((uint64_t)(w.v[0] >> 6) << 26) | (uint64_t)(w.v[1] >> 6);
    return (double)(2 * v + 1) * (1.0 / 9007199254740992.0);
}

// smallest i with cdf[i] > target, clamped to m - 1; at most ceil(log2 m) probes whatever cdf holds
__host__ __device__ __forceinline__ int bpf_search(const double* cdf, int m, double target) {
    int lo = 0, hi = m - 1;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (cdf[mid] > target) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__host__ __device__ __forceinline__ int bpf_ancestor(const double* cdf, int m, uint64_t seed, int64_t j, int64_t obs) {
    return bpf_search(cdf, m, bpf_uniform(seed, j, obs) * cdf[m - 1]);
}

__host__ __device__ __forceinline__ int clamp_slot(int a, int m) { return a < 0 ? 0 : (a >= m ? m - 1 : a); }

// the trajectory of final particle j: walk the ancestors back from the last observation
__host__ __device__ __forceinline__ void bpf_traceback_one(const float* S, int64_t s_st, int64_t s_sp, const int32_t* anc, int m,
                                                           int n_obs, int step, int d, int j, float* out) {
    float* o = out + (int64_t)j * ((int64_t)n_obs * step + 1) * d;
    int i = j;
    for (int k = n_obs - 1; k >= 0; --k) {
        i = clamp_slot(anc[(int64_t)k * m + i], m);
        for (int t = k * step + 1; t <= (k + 1) * step; ++t)
            for (int c = 0; c < d; ++c) o[(int64_t)t * d + c] = S[t * s_st + i * s_sp + c];
    }
    for (int c = 0; c < d; ++c) o[c] = S[i * s_sp + c];
}

// log p(x_next | x) of a small-state chain (NoisyLorenz63.log_prob, sda/mcs.py:184-185)
template <int KIND>
__host__ __device__ __forceinline__ double chain_pair_log_prob(const sda_chain_model& m, const float* x, const float* x_next) {
    using Sys = typename ChainSmall<KIND>::Sys;
    float mu[Sys::N];
#pragma unroll
    for (int c = 0; c < Sys::N; ++c) mu[c] = x[c];
    rk4_transition(Sys{m.p}, m.h, m.steps, mu);
    double l = 0.0;
#pragma unroll
    for (int c = 0; c < Sys::N; ++c) l += normal_log_prob((double)x_next[c], (double)mu[c], (double)m.noise_std);
    return l;
}

// pair (x, x_next) of a trajectory: returns log p(x_next | x) exactly as chain_pair_log_prob does, r = (x_next - T(x)) / noise_std^2
// (= d log p / d T(x) = -d log p / d x_next) and jtr = J_T(x)^T r (= d log p / d x)
template <int KIND>
__host__ __device__ __forceinline__ double chain_pair_residual(const sda_chain_model& m, const float* x, const float* x_next, float* r,
                                                               float* jtr) {
    using Sys = typename ChainSmall<KIND>::Sys;
    const Sys sys{m.p};
    float mu[Sys::N];
#pragma unroll
    for (int c = 0; c < Sys::N; ++c) mu[c] = x[c];
    rk4_transition(sys, m.h, m.steps, mu);
    double l = 0.0;
#pragma unroll
    for (int c = 0; c < Sys::N; ++c) l += normal_log_prob((double)x_next[c], (double)mu[c], (double)m.noise_std);
    const float s2 = m.noise_std * m.noise_std;
#pragma unroll
    for (int c = 0; c < Sys::N; ++c) { r[c] = (x_next[c] - mu[c]) / s2; jtr[c] = r[c]; }
    rk4_transition_vjp(sys, m.h, m.steps, x, jtr);
    return l;
}

static int chain_model_check(const sda_chain_model* m) {
    if (!m || m->steps < 1 || !(m->noise_std >= 0.f)) return SDA_E_BADARG;
    if (m->kind == SDA_CHAIN_LORENZ63) return m->d == 3 ? SDA_OK : SDA_E_BADARG;
    if (m->kind == SDA_CHAIN_LOTKA_VOLTERRA) return m->d == 2 ? SDA_OK : SDA_E_BADARG;
    if (m->kind == SDA_CHAIN_LORENZ96) return m->d >= 4 && m->d <= 64 ? SDA_OK : SDA_E_UNSUPPORTED;
    return SDA_E_UNSUPPORTED;
}

static int chain_adv_check(const sda_chain_adv* a) {
    if (!a) return SDA_E_BADARG;
    int rc = chain_model_check(&a->model);
    if (rc != SDA_OK) return rc;
    if (!a->x_in || !a->out || a->m < 1 || a->transitions < 1 || a->row0 < 0 || a->draw0 < 0) return SDA_E_BADARG;
    if (a->in_sp < a->model.d || a->out_sp < a->model.d) return SDA_E_BADARG;
    if (a->obs) {
        if (a->model.kind == SDA_CHAIN_LORENZ96) return SDA_E_UNSUPPORTED;
        if (!a->logw || !a->pmax) return SDA_E_BADARG;
        return chain_obs_check(a->obs, a->model.d);
    }
    return SDA_OK;
}

static int chain_vjp_check(const sda_chain_vjp* a) {
    if (!a) return SDA_E_BADARG;
    int rc = chain_model_check(&a->model);
    if (rc != SDA_OK) return rc;
    if (a->anc) return SDA_E_UNSUPPORTED;       // the particle filter's ancestor gather is not differentiated
    if (!a->x_in || !a->g || !a->gx || a->m < 1 || a->transitions < 1 || (a->transitions > 1 && !a->states)) return SDA_E_BADARG;
    const int d = a->model.d;
    if (a->in_sp < d || a->g_sp < d || a->gx_sp < d || (a->states && (a->st_sp < d || a->st_st < 0))) return SDA_E_BADARG;
    if (a->every && a->g_st < 0) return SDA_E_BADARG;
    return SDA_OK;
}

static int chain_lp_check(const sda_chain_model* model, const float* x, int b, int len, int64_t sl, const double* out) {
    int rc = chain_model_check(model);
    if (rc != SDA_OK) return rc;
    if (model->kind == SDA_CHAIN_LORENZ96) return SDA_E_UNSUPPORTED;
    if (!x || !out || b < 1 || len < 2 || sl < model->d || !(model->noise_std > 0.f)) return SDA_E_BADARG;
    return SDA_OK;
}

static int chain_lpg_check(const sda_chain_model* model, const float* x, int b, int len, int64_t sl, const double* out,
                           const float* grad) {
    int rc = chain_lp_check(model, x, b, len, sl, out);
    return rc != SDA_OK ? rc : (grad ? SDA_OK : SDA_E_BADARG);
}

extern "C" int sda_bpf_logweights_blocks(int m) { return m < 1 ? SDA_E_BADARG : (m + CH_THREADS - 1) / CH_THREADS; }

#ifndef SDA_HOST_EMU
// ---------------------------------------------------------------- device kernels
// launch KERNEL<kind> for one of the two small-state kinds (the checks have refused every other kind for these entries) on
// ceil(items / per_block) workgroups
#define CHAIN_LAUNCH_SMALL(kind, KERNEL, items, per_block, stream, ...)                                                        \
    do {                                                                                                                       \
        const dim3 grid((unsigned)(((items) + (per_block) - 1) / (per_block)));                                                \
        if ((kind) == SDA_CHAIN_LORENZ63)                                                                                      \
            hipLaunchKernelGGL(KERNEL<SDA_CHAIN_LORENZ63>, grid, dim3(CH_THREADS), 0, stream, __VA_ARGS__);                    \
        else                                                                                                                   \
            hipLaunchKernelGGL(KERNEL<SDA_CHAIN_LOTKA_VOLTERRA>, grid, dim3(CH_THREADS), 0, stream, __VA_ARGS__);              \
    } while (0)

// the Lorenz-96 launch: sub-groups of W lanes (W = next power of two >= d, at least 4), CH_THREADS / W particles per workgroup
static int chain_l96_geometry(int d, int m, int* W, unsigned* blocks) {
    int w = 4;
    while (w < d) w <<= 1;
    const int per_block = CH_THREADS / w;
    const int64_t nb = ((int64_t)m + per_block - 1) / per_block;
    if (nb > 0x7fffffff) return SDA_E_UNSUPPORTED;
    *W = w;
    *blocks = (unsigned)nb;
    return SDA_OK;
}

struct ChainAdvArgs {       // sda_chain_adv without the host pointer
    sda_chain_model model;
    const float* x_in; int64_t in_sp; const int32_t* anc;
    float* out; int64_t out_st, out_sp; int32_t every, m, transitions;
    uint64_t seed; int64_t row0, draw0;
    int32_t has_obs; float* logw; float* pmax;
};

// max over the workgroup's CH_THREADS values -> pmax[blockIdx.x] (every thread of the workgroup calls it)
__device__ __forceinline__ void block_max_store(float v, float* pmax) {
    __shared__ float s_max[CH_THREADS / SDA_WAVE];
    v = sda_wave_max(v);
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        float r = s_max[0];
#pragma unroll
        for (int w = 1; w < CH_THREADS / SDA_WAVE; ++w) r = fmaxf(r, s_max[w]);
        pmax[blockIdx.x] = r;
    }
}

template <int KIND>
__global__ __launch_bounds__(CH_THREADS) void chain_advance_small_kernel(ChainAdvArgs a, sda_chain_obs obs) {
    using Sys = typename ChainSmall<KIND>::Sys;
    const int j = blockIdx.x * CH_THREADS + threadIdx.x;
    const bool live = j < a.m;
    float x[Sys::N];
#pragma unroll
    for (int c = 0; c < Sys::N; ++c) x[c] = 0.f;
    if (live) {
        const int src = a.anc ? clamp_slot(a.anc[j], a.m) : j;
#pragma unroll
        for (int c = 0; c < Sys::N; ++c) x[c] = a.x_in[src * a.in_sp + c];
        for (int t = 0; t < a.transitions; ++t) {
            rk4_transition(Sys{a.model.p}, a.model.h, a.model.steps, x);
            if (a.model.noise_std > 0.f) {
                float z[4];
                chain_noise4(a.seed, (uint64_t)(a.row0 + j), a.draw0 + t, 0, z);
#pragma unroll
                for (int c = 0; c < Sys::N; ++c) x[c] = x[c] + a.model.noise_std * z[c];
            }
            if (a.every) {
#pragma unroll
                for (int c = 0; c < Sys::N; ++c) a.out[t * a.out_st + j * a.out_sp + c] = x[c];
            }
        }
        if (!a.every) {
#pragma unroll
            for (int c = 0; c < Sys::N; ++c) a.out[j * a.out_sp + c] = x[c];
        }
    }
    if (a.has_obs) {        // wave-uniform: the whole workgroup takes it
        float l = -INFINITY;
        if (live) {
            l = obs_logweight(obs, obs.y, x);
            a.logw[j] = l;
        }
        block_max_store(l, a.pmax);
    }
}

// Lorenz-96: component c of a particle on lane (group base + c) of a sub-group of W lanes, W = next power of two >= n
__global__ __launch_bounds__(CH_THREADS) void chain_advance_l96_kernel(ChainAdvArgs a, int W) {
    const int n = a.model.d;
    const int lane = threadIdx.x & 63, sub = lane & (W - 1), base = lane - sub;
    const int per_block = CH_THREADS / W;
    const int64_t j = (int64_t)blockIdx.x * per_block + threadIdx.x / W;
    const bool live = j < a.m && sub < n;
    const int c = sub < n ? sub : 0;
    const L96LaneSys sys{l96_lanes(base, c, n), a.model.p[0]};
    float x = 0.f;
    if (live) {
        const int64_t src = a.anc ? clamp_slot(a.anc[j], a.m) : j;
        x = a.x_in[src * a.in_sp + c];
    }
    // every lane of the wave runs the shuffles (dead lanes carry zeros); only the stores are predicated
    for (int t = 0; t < a.transitions; ++t) {
        rk4_transition(sys, a.model.h, a.model.steps, &x);
        if (a.model.noise_std > 0.f && live) {
            float z[4];
            chain_noise4(a.seed, (uint64_t)(a.row0 + j), a.draw0 + t, c >> 2, z);
            x = x + a.model.noise_std * z[c & 3];
        }
        if (a.every && live) a.out[t * a.out_st + j * a.out_sp + c] = x;
    }
    if (!a.every && live) a.out[j * a.out_sp + c] = x;
}

extern "C" int sda_chain_advance(const sda_chain_adv* a, void* stream) {
    int rc = chain_adv_check(a);
    if (rc != SDA_OK) return rc;
    ChainAdvArgs k;
    k.model = a->model;
    k.x_in = a->x_in; k.in_sp = a->in_sp; k.anc = a->anc;
    k.out = a->out; k.out_st = a->every ? a->out_st : 0; k.out_sp = a->out_sp;
    k.every = a->every ? 1 : 0; k.m = a->m; k.transitions = a->transitions;
    k.seed = a->seed; k.row0 = a->row0; k.draw0 = a->draw0;
    k.has_obs = a->obs ? 1 : 0; k.logw = a->logw; k.pmax = a->pmax;
    sda_chain_obs obs = {};
    if (a->obs) obs = *a->obs;
    const hipStream_t st = (hipStream_t)stream;
    if (a->model.kind == SDA_CHAIN_LORENZ96) {
        int W;
        unsigned blocks;
        rc = chain_l96_geometry(a->model.d, a->m, &W, &blocks);
        if (rc != SDA_OK) return rc;
        hipLaunchKernelGGL(chain_advance_l96_kernel, dim3(blocks), dim3(CH_THREADS), 0, st, k, W);
    } else {
        CHAIN_LAUNCH_SMALL(a->model.kind, chain_advance_small_kernel, a->m, CH_THREADS, st, k, obs);
    }
    return sda_launch_status();
}

// ---------------------------------------------------------------- the adjoint of sda_chain_advance: one launch walks every
// transition backwards.  The geometry is the forward's (one particle per lane / per sub-group), a particle's cotangent never leaves
// its lane or sub-group and nothing is accumulated across particles: no atomics, and a row does not depend on m.
struct ChainVjpArgs {       // sda_chain_vjp without anc
    sda_chain_model model;
    const float* x_in; int64_t in_sp;
    const float* states; int64_t st_st, st_sp;
    const float* g; int64_t g_st, g_sp;
    float* gx; int64_t gx_sp;
    int32_t every, m, transitions;
};

template <int KIND>
__global__ __launch_bounds__(CH_THREADS) void chain_advance_vjp_small_kernel(ChainVjpArgs a) {
    using Sys = typename ChainSmall<KIND>::Sys;
    const int j = blockIdx.x * CH_THREADS + threadIdx.x;
    if (j >= a.m) return;
    const int T = a.transitions;
    float g[Sys::N], x0[Sys::N];
#pragma unroll
    for (int c = 0; c < Sys::N; ++c) g[c] = a.g[(a.every ? (T - 1) * a.g_st : 0) + j * a.g_sp + c];
    for (int t = T - 1; t >= 0; --t) {
        const float* xs = t ? a.states + (t - 1) * a.st_st + j * a.st_sp : a.x_in + j * a.in_sp;
#pragma unroll
        for (int c = 0; c < Sys::N; ++c) x0[c] = xs[c];
        rk4_transition_vjp(Sys{a.model.p}, a.model.h, a.model.steps, x0, g);
        if (a.every && t) {
#pragma unroll
            for (int c = 0; c < Sys::N; ++c) g[c] = a.g[(t - 1) * a.g_st + j * a.g_sp + c] + g[c];
        }
    }
#pragma unroll
    for (int c = 0; c < Sys::N; ++c) a.gx[j * a.gx_sp + c] = g[c];
}

__global__ __launch_bounds__(CH_THREADS) void chain_advance_vjp_l96_kernel(ChainVjpArgs a, int W) {
    const int n = a.model.d;
    const int lane = threadIdx.x & 63, sub = lane & (W - 1), base = lane - sub;
    const int per_block = CH_THREADS / W;
    const int64_t j = (int64_t)blockIdx.x * per_block + threadIdx.x / W;
    const bool live = j < a.m && sub < n;
    const int c = sub < n ? sub : 0;
    const L96LaneSys sys{l96_lanes(base, c, n), a.model.p[0]};
    const int T = a.transitions;
    float g = 0.f;
    if (live) g = a.g[(a.every ? (T - 1) * a.g_st : 0) + j * a.g_sp + c];
    // every lane of the wave runs the shuffles (dead lanes carry zeros); the trip counts depend on the model alone
    for (int t = T - 1; t >= 0; --t) {
        float x0 = 0.f;
        if (live) x0 = t ? a.states[(t - 1) * a.st_st + j * a.st_sp + c] : a.x_in[j * a.in_sp + c];
        rk4_transition_vjp(sys, a.model.h, a.model.steps, &x0, &g);
        if (a.every && t && live) g = a.g[(t - 1) * a.g_st + j * a.g_sp + c] + g;
    }
    if (live) a.gx[j * a.gx_sp + c] = g;
}

extern "C" int sda_chain_advance_vjp(const sda_chain_vjp* a, void* stream) {
    int rc = chain_vjp_check(a);
    if (rc != SDA_OK) return rc;
    ChainVjpArgs k;
    k.model = a->model;
    k.x_in = a->x_in; k.in_sp = a->in_sp;
    k.states = a->states; k.st_st = a->st_st; k.st_sp = a->st_sp;
    k.g = a->g; k.g_st = a->every ? a->g_st : 0; k.g_sp = a->g_sp;
    k.gx = a->gx; k.gx_sp = a->gx_sp;
    k.every = a->every ? 1 : 0; k.m = a->m; k.transitions = a->transitions;
    const hipStream_t st = (hipStream_t)stream;
    if (a->model.kind == SDA_CHAIN_LORENZ96) {
        int W;
        unsigned blocks;
        rc = chain_l96_geometry(a->model.d, a->m, &W, &blocks);
        if (rc != SDA_OK) return rc;
        hipLaunchKernelGGL(chain_advance_vjp_l96_kernel, dim3(blocks), dim3(CH_THREADS), 0, st, k, W);
    } else {
        CHAIN_LAUNCH_SMALL(a->model.kind, chain_advance_vjp_small_kernel, a->m, CH_THREADS, st, k);
    }
    return sda_launch_status();
}

// value and gradient of sda_chain_log_prob: one wave per trajectory, lanes stride over the time indices.  The lane that owns index
// i evaluates pair (i, i + 1): its log-density (summed exactly as chain_log_prob_kernel sums it), r_i and J_T(x_i)^T r_i; r_{i-1}
// comes from the lane below, and for lane 0 from lane 63 of the previous stride.  Gather form: one store per element, no atomics.
template <int KIND>
__global__ __launch_bounds__(CH_THREADS) void chain_log_prob_grad_kernel(sda_chain_model model, const float* __restrict__ x, int b,
                                                                         int len, int64_t sb, int64_t sl, double* __restrict__ out,
                                                                         float* __restrict__ grad) {
    using Sys = typename ChainSmall<KIND>::Sys;
    const int lane = threadIdx.x & 63;
    const int traj = blockIdx.x * (CH_THREADS / SDA_WAVE) + (threadIdx.x >> 6);
    const bool have = traj < b;                // the same in every lane of the wave
    const float* xt = x + traj * sb;
    float* gt = grad + (int64_t)traj * len * Sys::N;
    double acc = 0.0;
    float carry[Sys::N];
#pragma unroll
    for (int c = 0; c < Sys::N; ++c) carry[c] = 0.f;
    for (int i0 = 0; i0 < len; i0 += SDA_WAVE) {        // every lane takes every trip: the shuffles below need the whole wave
        const int i = i0 + lane;
        float r[Sys::N], jtr[Sys::N];
#pragma unroll
        for (int c = 0; c < Sys::N; ++c) { r[c] = 0.f; jtr[c] = 0.f; }
        if (have && i + 1 < len) {
            float p[Sys::N], q[Sys::N];
#pragma unroll
            for (int c = 0; c < Sys::N; ++c) { p[c] = xt[i * sl + c]; q[c] = xt[(i + 1) * sl + c]; }
            acc += chain_pair_residual<KIND>(model, p, q, r, jtr);
        }
#pragma unroll
        for (int c = 0; c < Sys::N; ++c) {
            const float below = __shfl_up(r[c], 1, SDA_WAVE);
            const float prev = lane ? below : carry[c];
            carry[c] = __shfl(r[c], SDA_WAVE - 1, SDA_WAVE);
            if (have && i < len) gt[(int64_t)i * Sys::N + c] = jtr[c] - prev;
        }
    }
    acc = sda_wave_sum(acc);
    if (lane == 0 && have) out[traj] = acc;
}

extern "C" int sda_chain_log_prob_grad(const sda_chain_model* model, const float* x, int b, int len, int64_t sb, int64_t sl,
                                       double* out, float* grad, void* stream) {
    int rc = chain_lpg_check(model, x, b, len, sl, out, grad);
    if (rc != SDA_OK) return rc;
    CHAIN_LAUNCH_SMALL(model->kind, chain_log_prob_grad_kernel, b, CH_THREADS / SDA_WAVE, (hipStream_t)stream, *model, x, b, len, sb, sl,
                       out, grad);
    return sda_launch_status();
}

// one wave per trajectory: lanes stride over the L - 1 pairs, float64 partial sums, one shuffle tree
template <int KIND>
__global__ __launch_bounds__(CH_THREADS) void chain_log_prob_kernel(sda_chain_model model, const float* __restrict__ x, int b, int len,
                                                                    int64_t sb, int64_t sl, double* __restrict__ out) {
    using Sys = typename ChainSmall<KIND>::Sys;
    const int lane = threadIdx.x & 63;
    const int traj = blockIdx.x * (CH_THREADS / SDA_WAVE) + (threadIdx.x >> 6);
    double acc = 0.0;
    if (traj < b) {
        const float* xt = x + traj * sb;
        for (int i = lane; i + 1 < len; i += SDA_WAVE) {
            float a[Sys::N], n[Sys::N];
#pragma unroll
            for (int c = 0; c < Sys::N; ++c) { a[c] = xt[i * sl + c]; n[c] = xt[(i + 1) * sl + c]; }
            acc += chain_pair_log_prob<KIND>(model, a, n);
        }
    }
    acc = sda_wave_sum(acc);
    if (lane == 0 && traj < b) out[traj] = acc;
}

extern "C" int sda_chain_log_prob(const sda_chain_model* model, const float* x, int b, int len, int64_t sb, int64_t sl, double* out,
                                  void* stream) {
    int rc = chain_lp_check(model, x, b, len, sl, out);
    if (rc != SDA_OK) return rc;
    CHAIN_LAUNCH_SMALL(model->kind, chain_log_prob_kernel, b, CH_THREADS / SDA_WAVE, (hipStream_t)stream, *model, x, b, len, sb, sl, out);
    return sda_launch_status();
}

__global__ __launch_bounds__(CH_THREADS) void bpf_logweights_kernel(const float* __restrict__ x, int m, int64_t sp, sda_chain_obs obs,
                                                                    float* __restrict__ logw, float* __restrict__ pmax) {
    const int j = blockIdx.x * CH_THREADS + threadIdx.x;
    float l = -INFINITY;
    if (j < m) {
        l = obs_logweight(obs, obs.y, x + j * sp);
        logw[j] = l;
    }
    block_max_store(l, pmax);
}

extern "C" int sda_bpf_logweights(const float* x, int m, int64_t sp, int d, const sda_chain_obs* obs, float* logw, float* pmax,
                                  void* stream) {
    if (!x || !logw || !pmax || m < 1 || d < 1 || sp < d) return SDA_E_BADARG;
    int rc = chain_obs_check(obs, d);
    if (rc != SDA_OK) return rc;
    hipLaunchKernelGGL(bpf_logweights_kernel, dim3((unsigned)((m + CH_THREADS - 1) / CH_THREADS)), dim3(CH_THREADS), 0,
                       (hipStream_t)stream, x, m, sp, *obs, logw, pmax);
    return sda_launch_status();
}

// ONE workgroup: max (+ NaN / all -inf check), then the vector in chunks of CDF_THREADS with a float64 carry.  The chunk loop
// has a trip count every thread computes from m alone, so the barriers inside it are uniform.
#define CDF_THREADS 1024
__global__ __launch_bounds__(CDF_THREADS) void bpf_cdf_kernel(const float* __restrict__ logw, int m, const float* __restrict__ pmax,
                                                              int npmax, float* __restrict__ w, double* __restrict__ cdf,
                                                              int32_t* __restrict__ status) {
    __shared__ float s_max[CDF_THREADS / SDA_WAVE];
    __shared__ int s_bad[CDF_THREADS / SDA_WAVE];
    __shared__ double s_sum[CDF_THREADS / SDA_WAVE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float mx = -INFINITY;
    int bad = 0;
    for (int i = tid; i < m; i += CDF_THREADS) {
        const float l = logw[i];
        bad |= (l != l);
        if (!pmax) mx = fmaxf(mx, l);
    }
    if (pmax)
        for (int i = tid; i < npmax; i += CDF_THREADS) mx = fmaxf(mx, pmax[i]);
    mx = sda_wave_max(mx);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bad |= __shfl_down(bad, off, SDA_WAVE);
    if (lane == 0) { s_max[wave] = mx; s_bad[wave] = bad; }
    __syncthreads();
    mx = s_max[0]; bad = s_bad[0];
#pragma unroll
    for (int k = 1; k < CDF_THREADS / SDA_WAVE; ++k) { mx = fmaxf(mx, s_max[k]); bad |= s_bad[k]; }
    const bool degenerate = bad || !(mx > -INFINITY) || !(mx < INFINITY);      // the same value in every thread
    if (tid == 0) status[0] = degenerate ? 1 : 0;
    if (degenerate) {
        for (int i = tid; i < m; i += CDF_THREADS) { w[i] = 1.0f; cdf[i] = (double)(i + 1); }
        return;
    }
    double carry = 0.0;
    const int chunks = (m + CDF_THREADS - 1) / CDF_THREADS;
    for (int ch = 0; ch < chunks; ++ch) {
        const int i = ch * CDF_THREADS + tid;
        float wi = 0.f;
        if (i < m) { wi = expf(logw[i] - mx); w[i] = wi; }
        double v = (double)wi;
#pragma unroll
        for (int off = 1; off < SDA_WAVE; off <<= 1) {      // inclusive scan inside the wave
            const double u = __shfl_up(v, off, SDA_WAVE);
            if (lane >= off) v += u;
        }
        if (lane == 63) s_sum[wave] = v;
        __syncthreads();
        double before = carry, total = 0.0;
#pragma unroll
        for (int k = 0; k < CDF_THREADS / SDA_WAVE; ++k) {
            const double s = s_sum[k];
            if (k < wave) before += s;
            total += s;
        }
        if (i < m) cdf[i] = before + v;
        carry += total;
        __syncthreads();        // s_sum is rewritten by the next chunk
    }
}

extern "C" int sda_bpf_cdf(const float* logw, int m, const float* pmax, int npmax, float* w, double* cdf, int32_t* status,
                           void* stream) {
    if (!logw || !w || !cdf || !status || m < 1 || (pmax && npmax < 1)) return SDA_E_BADARG;
    hipLaunchKernelGGL(bpf_cdf_kernel, dim3(1), dim3(CDF_THREADS), 0, (hipStream_t)stream, logw, m, pmax, npmax, w, cdf, status);
    return sda_launch_status();
}

__global__ __launch_bounds__(CH_THREADS) void bpf_resample_kernel(const double* __restrict__ cdf, int m, uint64_t seed, int64_t obs,
                                                                  int32_t* __restrict__ anc) {
    const int j = blockIdx.x * CH_THREADS + threadIdx.x;
    if (j < m) anc[j] = bpf_ancestor(cdf, m, seed, j, obs);
}

extern "C" int sda_bpf_resample(const double* cdf, int m, uint64_t seed, int64_t obs_index, int32_t* anc, void* stream) {
    if (!cdf || !anc || m < 1 || obs_index < 0) return SDA_E_BADARG;
    hipLaunchKernelGGL(bpf_resample_kernel, dim3((unsigned)((m + CH_THREADS - 1) / CH_THREADS)), dim3(CH_THREADS), 0,
                       (hipStream_t)stream, cdf, m, seed, obs_index, anc);
    return sda_launch_status();
}

__global__ __launch_bounds__(CH_THREADS) void bpf_traceback_kernel(const float* __restrict__ S, int64_t s_st, int64_t s_sp,
                                                                   const int32_t* __restrict__ anc, int m, int n_obs, int step, int d,
                                                                   float* __restrict__ out) {
    const int j = blockIdx.x * CH_THREADS + threadIdx.x;
    if (j < m) bpf_traceback_one(S, s_st, s_sp, anc, m, n_obs, step, d, j, out);
}

extern "C" int sda_bpf_traceback(const float* S, int64_t s_st, int64_t s_sp, const int32_t* anc, int m, int n_obs, int step, int d,
                                 float* out, void* stream) {
    if (!S || !anc || !out || m < 1 || n_obs < 1 || step < 1 || d < 1 || s_sp < d || s_st < 0) return SDA_E_BADARG;
    if ((int64_t)n_obs * step + 1 > 0x7fffffff) return SDA_E_UNSUPPORTED;
    hipLaunchKernelGGL(bpf_traceback_kernel, dim3((unsigned)((m + CH_THREADS - 1) / CH_THREADS)), dim3(CH_THREADS), 0,
                       (hipStream_t)stream, S, s_st, s_sp, anc, m, n_obs, step, d, out);
    return sda_launch_status();
}

#else  // SDA_HOST_EMU
// ---------------------------------------------------------------- CPU replay (tests only; libsda_emu.so): the same
// __host__ __device__ functions and the same RK4 templates inside plain loops over HOST arrays.  Lorenz-96 keeps a particle in
// one array (L96ArraySys) where the device keeps it on the lanes of a sub-group (L96LaneSys): the stage sequence is the one
// template, the neighbours are the one l96_lanes, only "index the array" stands where the device shuffles.

extern "C" int sda_chain_advance_host(const sda_chain_adv* a) {
    int rc = chain_adv_check(a);
    if (rc != SDA_OK) return rc;
    const sda_chain_model& md = a->model;
    const int d = md.d;
    for (int j = 0; j < a->m; ++j) {
        const int src = a->anc ? clamp_slot(a->anc[j], a->m) : j;
        float x[64];
        for (int c = 0; c < d; ++c) x[c] = a->x_in[src * a->in_sp + c];
        for (int t = 0; t < a->transitions; ++t) {
            if (md.kind == SDA_CHAIN_LORENZ63) rk4_transition(Lorenz63Sys{md.p}, md.h, md.steps, x);
            else if (md.kind == SDA_CHAIN_LOTKA_VOLTERRA) rk4_transition(LotkaVolterraSys{md.p}, md.h, md.steps, x);
            else rk4_transition(L96ArraySys{d, md.p[0]}, md.h, md.steps, x);
            if (md.noise_std > 0.f)
                for (int q = 0; 4 * q < d; ++q) {
                    float z[4];
                    chain_noise4(a->seed, (uint64_t)(a->row0 + j), a->draw0 + t, q, z);
                    for (int e = 0; e < 4 && 4 * q + e < d; ++e) x[4 * q + e] = x[4 * q + e] + md.noise_std * z[e];
                }
            if (a->every)
                for (int c = 0; c < d; ++c) a->out[t * a->out_st + j * a->out_sp + c] = x[c];
        }
        if (!a->every)
            for (int c = 0; c < d; ++c) a->out[j * a->out_sp + c] = x[c];
        if (a->obs) a->logw[j] = obs_logweight(*a->obs, a->obs->y, x);
    }
    return SDA_OK;
}

extern "C" int sda_chain_advance_vjp_host(const sda_chain_vjp* a) {
    int rc = chain_vjp_check(a);
    if (rc != SDA_OK) return rc;
    const sda_chain_model& md = a->model;
    const int d = md.d, T = a->transitions;
    for (int64_t j = 0; j < a->m; ++j) {
        float g[64], x0[64];
        for (int c = 0; c < d; ++c) g[c] = a->g[(a->every ? (T - 1) * a->g_st : 0) + j * a->g_sp + c];
        for (int t = T - 1; t >= 0; --t) {
            const float* xs = t ? a->states + (t - 1) * a->st_st + j * a->st_sp : a->x_in + j * a->in_sp;
            for (int c = 0; c < d; ++c) x0[c] = xs[c];
            if (md.kind == SDA_CHAIN_LORENZ63) rk4_transition_vjp(Lorenz63Sys{md.p}, md.h, md.steps, x0, g);
            else if (md.kind == SDA_CHAIN_LOTKA_VOLTERRA) rk4_transition_vjp(LotkaVolterraSys{md.p}, md.h, md.steps, x0, g);
            else rk4_transition_vjp(L96ArraySys{d, md.p[0]}, md.h, md.steps, x0, g);
            if (a->every && t)
                for (int c = 0; c < d; ++c) g[c] = a->g[(t - 1) * a->g_st + j * a->g_sp + c] + g[c];
        }
        for (int c = 0; c < d; ++c) a->gx[j * a->gx_sp + c] = g[c];
    }
    return SDA_OK;
}

extern "C" int sda_chain_log_prob_grad_host(const sda_chain_model* model, const float* x, int b, int len, int64_t sb, int64_t sl,
                                            double* out, float* grad) {
    int rc = chain_lpg_check(model, x, b, len, sl, out, grad);
    if (rc != SDA_OK) return rc;
    const int d = model->d;
    for (int t = 0; t < b; ++t) {
        double acc = 0.0;
        float prev[3] = {0.f, 0.f, 0.f};
        for (int i = 0; i < len; ++i) {
            float r[3] = {0.f, 0.f, 0.f}, jtr[3] = {0.f, 0.f, 0.f};
            const float* p = x + t * sb + i * sl;
            if (i + 1 < len)
                acc += model->kind == SDA_CHAIN_LORENZ63 ? chain_pair_residual<SDA_CHAIN_LORENZ63>(*model, p, p + sl, r, jtr)
                                                         : chain_pair_residual<SDA_CHAIN_LOTKA_VOLTERRA>(*model, p, p + sl, r, jtr);
            for (int c = 0; c < d; ++c) {
                grad[((int64_t)t * len + i) * d + c] = jtr[c] - prev[c];
                prev[c] = r[c];
            }
        }
        out[t] = acc;
    }
    return SDA_OK;
}

extern "C" int sda_chain_log_prob_host(const sda_chain_model* model, const float* x, int b, int len, int64_t sb, int64_t sl,
                                       double* out) {
    int rc = chain_lp_check(model, x, b, len, sl, out);
    if (rc != SDA_OK) return rc;
    for (int t = 0; t < b; ++t) {
        double acc = 0.0;
        for (int i = 0; i + 1 < len; ++i) {
            const float* a = x + t * sb + i * sl;
            acc += model->kind == SDA_CHAIN_LORENZ63 ? chain_pair_log_prob<SDA_CHAIN_LORENZ63>(*model, a, a + sl)
                                                     : chain_pair_log_prob<SDA_CHAIN_LOTKA_VOLTERRA>(*model, a, a + sl);
        }
        out[t] = acc;
    }
    return SDA_OK;
}

extern "C" int sda_bpf_logweights_host(const float* x, int m, int64_t sp, int d, const sda_chain_obs* obs, float* logw) {
    if (!x || !logw || m < 1 || d < 1 || sp < d) return SDA_E_BADARG;
    int rc = chain_obs_check(obs, d);
    if (rc != SDA_OK) return rc;
    for (int j = 0; j < m; ++j) logw[j] = obs_logweight(*obs, obs->y, x + j * sp);
    return SDA_OK;
}

extern "C" int sda_bpf_resample_host(const double* cdf, int m, uint64_t seed, int64_t obs_index, int32_t* anc) {
    if (!cdf || !anc || m < 1 || obs_index < 0) return SDA_E_BADARG;
    for (int j = 0; j < m; ++j) anc[j] = bpf_ancestor(cdf, m, seed, j, obs_index);
    return SDA_OK;
}

extern "C" int sda_bpf_traceback_host(const float* S, int64_t s_st, int64_t s_sp, const int32_t* anc, int m, int n_obs, int step,
                                      int d, float* out) {
    if (!S || !anc || !out || m < 1 || n_obs < 1 || step < 1 || d < 1 || s_sp < d || s_st < 0) return SDA_E_BADARG;
    for (int j = 0; j < m; ++j) bpf_traceback_one(S, s_st, s_sp, anc, m, n_obs, step, d, j, out);
    return SDA_OK;
}
#endif  // SDA_HOST_EMU
