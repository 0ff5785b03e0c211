// The denoising loss of the opt-in training route (sda/score.py:265-276; sda_amd.score.VPSDE.loss with a training.KeyedLossNoise) as two
// replayable launches around the network evaluation.  torch's route draws t and eps with its generator and forms mu(t) x + sigma(t) eps,
// the squared error and its mean with about fifteen small launches; neither the draws nor the step they belong to can be tied to a
// captured graph.  Here
//   sda_loss_perturb   t[b], eps[b][.] and xt[b][.] = mu(t[b]) x[b][.] + sigma(t[b]) eps[b][.] in ONE launch.  The draws are keyed: eps[b] is
//                      BY DEFINITION row row0 + b of sda_randn_rows(seed, draw = 2 s) and t[b] = ((w0 >> 8) + 0.5) 2^-24 with w0 = word 0 of
//                      the same generator at quad 0 of draw 2 s + 1 (philox.hpp: same counters, same Box-Muller), s = the training step, read
//                      from device memory when step_dev != NULL (a replayed graph advances it on the device).  mu / sigma: sda_vp_mu_sigma,
//                      the function behind sda_vp_schedule.  One workgroup per chunk of PB_CHUNK = 1024 elements of one row, one quad per
//                      thread: a 16-byte path where per_row % 4 == 0 and x / eps / xt are 16-byte aligned, a scalar tail otherwise.  No LDS,
//                      plain vector stores, one writer per element (t[b]: the thread that owns quad 0 of row b).
//   sda_loss_mse       loss[0] = mean((out - eps)^2) and, optionally, g = (2 / numel) (out - eps), the loss's cotangent at out.  Two ordered
//                      stages, no float atomics, no workgroup waits for another: (1) workgroup w sums chunk w of MSE_CHUNK = 4096 elements --
//                      every thread MSE_PER_THREAD = 16 terms in index order, a 64-lane shuffle tree, the four wave sums in wave order -- into
//                      work[w]; (2) ONE workgroup: thread i sums work[i], work[i + 256], ... in index order, then the same tree, and divides
//                      by numel.  The order of every addition is fixed by numel alone: bitwise reproducible.  sda_loss_mse_plan exports the
//                      geometry and the longest chain of additions a term passes through (the error bound of the tests).
// Each product, sum and difference is rounded on its own (the unit is compiled with -ffp-contract=off).
#include "sda_common.hpp"

#include "philox.hpp"

#define PB_THREADS 256
#define PB_CHUNK 1024            // elements of a row per workgroup: one quad per thread

#define MSE_THREADS 256
#define MSE_PER_THREAD 16
#define MSE_CHUNK (MSE_THREADS * MSE_PER_THREAD)

static inline bool tl_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---------------------------------------------------------------------------------------------- perturbation
__global__ __launch_bounds__(PB_THREADS) void loss_perturb_kernel(const float* __restrict__ x, int rows, int64_t per_row, int chunks,
                                                                  uint32_t k0, uint32_t k1, int64_t row0, int64_t step,
                                                                  const int64_t* __restrict__ step_dev, int alpha_kind, float eta,
                                                                  float k, int sigma_kind, int vec, float* __restrict__ t,
                                                                  float* __restrict__ eps, float* __restrict__ xt) {
    if (step_dev) step = step_dev[0];
    const int b = (int)(blockIdx.x / (unsigned)chunks);                 // (the grid holds exactly rows * chunks workgroups: b < rows)
    const int64_t q = (int64_t)(blockIdx.x - (unsigned)b * (unsigned)chunks) * PB_THREADS + threadIdx.x;
    if (4 * q >= per_row) return;
    const uint64_t grow = (uint64_t)(row0 + b);
    const int64_t draw = 2 * step;
    // t[b]: a uniform in (0, 1) from the top 24 bits of word 0, quad 0, draw 2 s + 1 (every thread of the row forms the same value)
    const philox4 wt = philox_noise_words(0, grow, draw + 1, k0, k1);
    const float tv = ((float)(wt.v[0] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    float mu, sg;
    sda_vp_mu_sigma(tv, alpha_kind, eta, k, sigma_kind, mu, sg);
    float z[4];
    philox_normal4(q, grow, draw, k0, k1, z);
    if (q == 0) t[b] = tv;
    const int64_t e0 = (int64_t)b * per_row + 4 * q;
    if (vec) {
        const float4 x4 = *reinterpret_cast<const float4*>(x + e0);
        const float4 o = make_float4(mu * x4.x + sg * z[0], mu * x4.y + sg * z[1], mu * x4.z + sg * z[2], mu * x4.w + sg * z[3]);
        *reinterpret_cast<float4*>(eps + e0) = make_float4(z[0], z[1], z[2], z[3]);
        *reinterpret_cast<float4*>(xt + e0) = o;
    } else {
        const int64_t left = per_row - 4 * q;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < left) {
                eps[e0 + e] = z[e];
                xt[e0 + e] = mu * x[e0 + e] + sg * z[e];
            }
    }
}

extern "C" int sda_loss_perturb(const float* x, int rows, int64_t per_row, uint64_t seed, int64_t row0, int64_t step,
                                const int64_t* step_dev, int alpha_kind, float eta, float k, int sigma_kind, float* t, float* eps,
                                float* xt, void* stream) {
    if (!x || !t || !eps || !xt || rows < 1 || per_row < 1 || row0 < 0 || step < 0) return SDA_E_BADARG;
    if (alpha_kind < 0 || alpha_kind > 2 || sigma_kind < 0 || sigma_kind > 2) return SDA_E_BADARG;
    const int64_t chunks = (per_row + PB_CHUNK - 1) / PB_CHUNK;
    if (chunks * rows > 0x7fffffffLL) return SDA_E_UNSUPPORTED;
    const int vec = (per_row & 3) == 0 && tl_aligned16(x) && tl_aligned16(eps) && tl_aligned16(xt);
    hipLaunchKernelGGL(loss_perturb_kernel, dim3((unsigned)(chunks * rows)), dim3(PB_THREADS), 0, (hipStream_t)stream, x, rows, per_row,
                       (int)chunks, (uint32_t)seed, (uint32_t)(seed >> 32), row0, step, step_dev, alpha_kind, eta, k, sigma_kind, vec, t,
                       eps, xt);
    return sda_launch_status();
}

// ---------------------------------------------------------------------------------------------- mean squared error + cotangent
// the workgroup's sum of one value per thread, valid in thread 0: 6 shuffle additions, then ((w0 + w1) + w2) + w3
__device__ __forceinline__ float mse_block_sum(float v, float* wave_sums) {
    v = sda_wave_sum(v);
    if ((threadIdx.x & (SDA_WAVE - 1)) == 0) wave_sums[threadIdx.x / SDA_WAVE] = v;
    __syncthreads();
    return ((wave_sums[0] + wave_sums[1]) + wave_sums[2]) + wave_sums[3];
}

__global__ __launch_bounds__(MSE_THREADS) void loss_mse_partial_kernel(const float* __restrict__ out, const float* __restrict__ eps,
                                                                       int64_t numel, float scale, int vec, float* __restrict__ g,
                                                                       float* __restrict__ work) {
    __shared__ float wave_sums[MSE_THREADS / SDA_WAVE];
    const int64_t c0 = (int64_t)blockIdx.x * MSE_CHUNK;
    float acc = 0.0f;
    if (vec) {
#pragma unroll
        for (int j = 0; j < MSE_PER_THREAD / 4; ++j) {
            const int64_t e = c0 + 4 * (int64_t)(j * MSE_THREADS + threadIdx.x);
            if (e < numel) {                                            // (numel % 4 == 0: the quad is whole)
                const float4 o = *reinterpret_cast<const float4*>(out + e), z = *reinterpret_cast<const float4*>(eps + e);
                const float d0 = o.x - z.x, d1 = o.y - z.y, d2 = o.z - z.z, d3 = o.w - z.w;
                acc += d0 * d0; acc += d1 * d1; acc += d2 * d2; acc += d3 * d3;
                if (g) *reinterpret_cast<float4*>(g + e) = make_float4(scale * d0, scale * d1, scale * d2, scale * d3);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < MSE_PER_THREAD; ++j) {
            const int64_t e = c0 + j * MSE_THREADS + threadIdx.x;
            if (e < numel) {
                const float d = out[e] - eps[e];
                acc += d * d;
                if (g) g[e] = scale * d;
            }
        }
    }
    const float s = mse_block_sum(acc, wave_sums);
    if (threadIdx.x == 0) work[blockIdx.x] = s;
}

__global__ __launch_bounds__(MSE_THREADS) void loss_mse_final_kernel(const float* __restrict__ work, int blocks, int64_t numel,
                                                                     float* __restrict__ loss) {
    __shared__ float wave_sums[MSE_THREADS / SDA_WAVE];
    float acc = 0.0f;
    for (int i = threadIdx.x; i < blocks; i += MSE_THREADS) acc += work[i];
    const float s = mse_block_sum(acc, wave_sums);
    if (threadIdx.x == 0) loss[0] = (float)((double)s / (double)numel);            // one rounding, also where numel > 2^24
}

// blocks of stage 1 (= floats of `work`) and the longest chain of additions a term passes through: MSE_PER_THREAD in its thread, 6 + 3 in its
// workgroup's tree, ceil(blocks / 256) in stage 2's thread, 6 + 3 in stage 2's tree.  Returns the floats of `work`, or SDA_E_* (< 0).
extern "C" int64_t sda_loss_mse_plan(int64_t numel, int* blocks, int* chain) {
    if (numel < 1) return SDA_E_BADARG;
    const int64_t nb = (numel + MSE_CHUNK - 1) / MSE_CHUNK;
    if (nb > 0x7fffffffLL) return SDA_E_UNSUPPORTED;
    if (blocks) *blocks = (int)nb;
    if (chain) *chain = MSE_PER_THREAD + 9 + (int)((nb + MSE_THREADS - 1) / MSE_THREADS) + 9;
    return nb;
}

extern "C" int sda_loss_mse(const float* out, const float* eps, int64_t numel, float* loss, float* g, float* work, void* stream) {
    if (!out || !eps || !loss || !work) return SDA_E_BADARG;
    int blocks = 0;
    const int64_t rc = sda_loss_mse_plan(numel, &blocks, nullptr);
    if (rc < 0) return (int)rc;
    const int vec = (numel & 3) == 0 && tl_aligned16(out) && tl_aligned16(eps) && (!g || tl_aligned16(g));
    const float scale = (float)(2.0 / (double)numel);
    hipLaunchKernelGGL(loss_mse_partial_kernel, dim3((unsigned)blocks), dim3(MSE_THREADS), 0, (hipStream_t)stream, out, eps, numel, scale,
                       vec, g, work);
    hipLaunchKernelGGL(loss_mse_final_kernel, dim3(1), dim3(MSE_THREADS), 0, (hipStream_t)stream, work, blocks, numel, loss);
    return sda_launch_status();
}
