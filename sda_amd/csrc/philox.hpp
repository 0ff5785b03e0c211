// Counter-based Philox4x32-10 (Salmon et al., SC'11; the generator behind torch's device RNG) + Box-Muller, shared by every keyed
// draw of the library: the row-keyed normals (noise.hip) and the kernels that regenerate them in place -- the keyed corrector
// (step1d.hip), the loss perturbation (train_loss.hip), the Markov chains and the particle filter (chain.hip), the linear-Gaussian
// model (lgss.hip) and the ensemble smoother (enks.hip), all through philox_normal4 -- and the window starts and epoch shuffles of
// the trajectory dataset (dataset.hip).
//
// Counter layouts in use (key = the 64-bit seed, low word first):
//   noise    element 4q..4q+3 of row r in draw t :  {q_lo, r_lo, t_lo, t_hi ^ (q_hi << 16) ^ (r_hi << 24)}
//   resample draw j of observation k             :  {j_lo, k_lo, 0x80000000 | j_hi, 0x52455341 ('RESA')}
//   window   start of row b in batch s           :  {b, s_lo, 0x80000000 | s_hi, 0x57535441 ('WSTA')}
//   shuffle  round r of value v in epoch e       :  {v, e_lo, 0x80000000 | e_hi, 0x53485530 ('SHU0') + r},  r = 0 .. 3
// A noise counter with t < 2^31 has bit 31 of word 2 clear, the other three have it set, and those differ in word 3 (s, e < 2^63:
// s_hi, e_hi < 2^31): no two layouts collide, so the dataset of a training run (dataset.hip) may reuse the seed of its loss noise.
#pragma once
#include <math.h>
#include <stdint.h>

#define PHILOX_M0 0xD2511F53u
#define PHILOX_M1 0xCD9E8D57u
#define PHILOX_W0 0x9E3779B9u
#define PHILOX_W1 0xBB67AE85u

struct philox4 { uint32_t v[4]; };

__host__ __device__ __forceinline__ philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                          uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += PHILOX_W0; k1 += PHILOX_W1;
    }
    philox4 o; o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
    return o;
}

// two uniforms in (0, 1) from the top 24 bits of each word (never 0 or 1) -> two independent N(0, 1)
__host__ __device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
    const float u1 = ((float)(a >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float u2 = ((float)(b >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincosf(6.28318530717958647692f * u2, &s, &c);
    z0 = r * c; z1 = r * s;
}

// the Philox words behind elements 4q .. 4q+3 of global row `grow` in draw `draw` (sda_randn_rows' counter)
__host__ __device__ __forceinline__ philox4 philox_noise_words(int64_t q, uint64_t grow, int64_t draw, uint32_t k0, uint32_t k1) {
    return philox4x32_10((uint32_t)q, (uint32_t)grow, (uint32_t)draw,
                         (uint32_t)((uint64_t)draw >> 32) ^ ((uint32_t)((uint64_t)q >> 32) << 16) ^
                             ((uint32_t)(grow >> 32) << 24),
                         k0, k1);
}

// THE four normals of quad q of global row `grow` in draw `draw`: what sda_randn_rows writes to elements 4q .. 4q+3 of that row.
// Every keyed-noise kernel draws through this one function, so they all see the same stream.
__host__ __device__ __forceinline__ void philox_normal4(int64_t q, uint64_t grow, int64_t draw, uint32_t k0, uint32_t k1, float* z) {
    const philox4 w = philox_noise_words(q, grow, draw, k0, k1);
    box_muller(w.v[0], w.v[1], z[0], z[1]);
    box_muller(w.v[2], w.v[3], z[2], z[3]);
}

// word 0 behind the window start of row b in global batch s (the `window` counter)
__host__ __device__ __forceinline__ uint32_t philox_window_word(uint32_t b, int64_t s, uint32_t k0, uint32_t k1) {
    return philox4x32_10(b, (uint32_t)s, 0x80000000u | (uint32_t)((uint64_t)s >> 32), 0x57535441u, k0, k1).v[0];
}

// word 0 behind round r of the epoch-e shuffle at half-word v (the `shuffle` counter)
__host__ __device__ __forceinline__ uint32_t philox_shuffle_word(int r, uint32_t v, int64_t e, uint32_t k0, uint32_t k1) {
    return philox4x32_10(v, (uint32_t)e, 0x80000000u | (uint32_t)((uint64_t)e >> 32), 0x53485530u + (uint32_t)r, k0, k1).v[0];
}
