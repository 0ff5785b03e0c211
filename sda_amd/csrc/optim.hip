// The optimizer step of the opt-in training route (sda_amd.training.AdamW): a multi-tensor AdamW with decoupled weight decay that keeps
// the whole-MLP plan's packed weights valid.  A training step of the Lorenz local net is bound by launch latency (csrc/mlp_train.hip), and
// after its three backward launches the remaining cost was torch's per-tensor optimizer launches plus the re-pack of the plan's slabs
// that every parameter change triggered (sda_amd/mlp.py _FusedPlan._pack: some ten tensor operations per GEMM, forward and transposed).
// Here ONE launch updates up to SDA_ADAMW_MAXT tensors (LOCAL_CONFIG: 14 GEMMs = 28 tensors + the time embedding's 4 = 32) and, for a tensor
// that is a GEMM weight or bias of a plan, also writes the new value to its place in the forward slab, the transposed slab or the
// padded bias row, so no re-pack follows.
//   * workgroup b owns ONE chunk of AO_CHUNK = 1024 consecutive elements of one tensor (blk0: block-prefix table, decoded by a
//     wave-uniform search on blockIdx.x: the per-tensor pointers come out of the kernel arguments through scalar loads);
//   * 256 threads, one float4 of p / g / m / v per thread (16 B per lane, consecutive lanes on consecutive addresses) where the tensor's
//     numel is a multiple of 4 and its four pointers are 16-byte aligned; otherwise four scalar elements per thread, 256 apart, so that
//     consecutive lanes still read consecutive addresses (in_f = 47 / 15: the rows of dw out of sda_mlp_wgrad are unaligned);
//   * a few registers and no LDS: occupancy is bounded by the block size alone.  LOCAL_CONFIG is 690 k elements = 680 workgroups of
//     4 waves on 256 CUs; the launch is latency-, not bandwidth-bound (14 MB of traffic), so one chunk per workgroup and no grid stride;
//   * plain vector stores only, every output element (p, m, v, slab positions) has exactly one writer: bitwise reproducible.
// sda_adamw_step_dev is the same launch for a replayed (hipGraph) training step: the three scalars that change from step to step -- decay,
// step_size, rsqrt_bc2 -- come from row irow[0] of a device table instead of the descriptor (sda_amd.training.GraphedStep).
// The element update and the slab position are __host__ __device__; the emulator at the bottom (libsda_emu.so, tests only) runs the same
// per-thread function on the host.
#include "sda_common.hpp"
#include <math.h>

#define AO_THREADS 256
#define AO_CHUNK 1024            // elements per workgroup: one float4 per thread

// ---------------------------------------------------------------- slab position (host + device); sda_amd/mlp.py _unit / _slab
__host__ __device__ inline int ao_mf(int out_f) { return out_f <= 16 ? 1 : (out_f <= 128 ? 8 : 16); }                      // D fragments of 16 features
__host__ __device__ inline int ao_kq(int in_f) { return in_f <= 16 ? 1 : (in_f <= 64 ? 4 : (in_f <= 128 ? 8 : 16)); }      // K quads of 16 values

// float offset of W[r][c], W [rows][cols] (rows = the GEMM's outputs, cols = its contraction), inside the slab of that GEMM: Wp = W zero
// padded to [16 mf][16 kq] is cut into units of at most 128 x 128 in the order [row half][column half], each padded to whole 4096-float
// pieces; inside a unit [fragment m][k quad sq][lane = 16 k + li][e] holds Wp[16 m + li][16 sq + 4 k + e]
__host__ __device__ inline int sda_mlp_slab_pos(int rows, int cols, int r, int c) {
    const int R = 16 * ao_mf(rows), C = 16 * ao_kq(cols);
    const int ur = R < 128 ? R : 128, uc = C < 128 ? C : 128;          // a unit's sides
    const int unit = (ur * uc + 4095) & ~4095;
    const int rr = r & 127, cc = c & 127;                               // (r < R, c < C: r >> 7 / c >> 7 = the half, 0 when that side has one)
    const int m = rr >> 4, li = rr & 15, sq = cc >> 4, k = (cc >> 2) & 3, e = cc & 3;
    return ((r >> 7) * (C / uc) + (c >> 7)) * unit + ((((m * (uc >> 4) + sq) * 4 + k) * 16 + li) * 4 + e);
}

// ---------------------------------------------------------------- the element update (host + device)
// torch's single-tensor AdamW, operation by operation (mul_, lerp_, mul_ + addcmul_, sqrt / bias correction + eps, addcdiv_); every product
// and sum is rounded on its own (the unit is compiled with -ffp-contract=off on both sides)
// the three scalars that change with the step count and the learning rate: by value in the descriptor (sda_adamw_step) or a row of a
// device table (sda_adamw_step_dev)
struct ao_step { float decay, step_size, rsqrt_bc2; };

__host__ __device__ inline void ao_update(const sda_adamw_desc& d, const ao_step& s, float g, float& p, float& m, float& v) {
    p = p * s.decay;
    m = m + (g - m) * d.one_m_beta1;
    v = v * d.beta2 + (d.one_m_beta2 * g) * g;
    const float denom = sqrtf(v) * s.rsqrt_bc2 + d.eps;
    p = p - s.step_size * (m / denom);
}

// the pack epilogue of element idx of a GEMM weight [out_f][in_f]
__host__ __device__ inline void ao_pack_weight(float* fwd, float* bwd, int out_f, int in_f, int o, int i, float p) {
    fwd[sda_mlp_slab_pos(out_f, in_f, o, i)] = p;
    bwd[sda_mlp_slab_pos(in_f, out_f, i, o)] = p;
}

__host__ __device__ inline bool ao_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// everything thread `tid` of workgroup `b` does
__host__ __device__ inline void ao_thread(const sda_adamw_desc& d, const ao_step& s, int b, int tid) {
    int t = 0;
    while (t + 1 < d.ntensor && b >= d.blk0[t + 1]) ++t;
    const int64_t e0 = (int64_t)(b - d.blk0[t]) * AO_CHUNK, numel = d.numel[t];
    float* const p = d.p[t];
    const float* const g = d.g[t];
    float* const m = d.m[t];
    float* const v = d.v[t];
    float* const fwd = d.fwd[t];
    float* const bwd = d.bwd[t];
    const int kind = d.pack_kind[t], out_f = d.out_f[t], in_f = d.in_f[t];
    if ((numel & 3) == 0 && ao_aligned16(p) && ao_aligned16(g) && ao_aligned16(m) && ao_aligned16(v)) {
        const int64_t e = e0 + 4 * tid;
        if (e >= numel) return;
        float4 p4 = *reinterpret_cast<const float4*>(p + e), m4 = *reinterpret_cast<const float4*>(m + e), v4 = *reinterpret_cast<const float4*>(v + e);
        const float4 g4 = *reinterpret_cast<const float4*>(g + e);
        ao_update(d, s, g4.x, p4.x, m4.x, v4.x);
        ao_update(d, s, g4.y, p4.y, m4.y, v4.y);
        ao_update(d, s, g4.z, p4.z, m4.z, v4.z);
        ao_update(d, s, g4.w, p4.w, m4.w, v4.w);
        *reinterpret_cast<float4*>(p + e) = p4;
        *reinterpret_cast<float4*>(m + e) = m4;
        *reinterpret_cast<float4*>(v + e) = v4;
        if (kind == 2) {
            if (ao_aligned16(fwd)) *reinterpret_cast<float4*>(fwd + e) = p4;
            else { fwd[e] = p4.x; fwd[e + 1] = p4.y; fwd[e + 2] = p4.z; fwd[e + 3] = p4.w; }
        } else if (kind == 1) {
            const float pv[4] = {p4.x, p4.y, p4.z, p4.w};
            int o = (int)(e / in_f), i = (int)(e - (int64_t)o * in_f);
            if ((in_f & 3) == 0 && ao_aligned16(fwd)) {
                // the four values stay in one row of W and are one lane's float4 of the forward slab (i % 4 == 0: element 0 of the lane)
                *reinterpret_cast<float4*>(fwd + sda_mlp_slab_pos(out_f, in_f, o, i)) = p4;
#pragma unroll
                for (int j = 0; j < 4; ++j) bwd[sda_mlp_slab_pos(in_f, out_f, i + j, o)] = pv[j];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    ao_pack_weight(fwd, bwd, out_f, in_f, o, i, pv[j]);
                    if (++i == in_f) { i = 0; ++o; }
                }
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < AO_CHUNK / AO_THREADS; ++j) {
        const int64_t e = e0 + j * AO_THREADS + tid;
        if (e >= numel) break;
        float pe = p[e], me = m[e], ve = v[e];
        ao_update(d, s, g[e], pe, me, ve);
        p[e] = pe; m[e] = me; v[e] = ve;
        if (kind == 2) fwd[e] = pe;
        else if (kind == 1) {
            const int o = (int)(e / in_f);
            ao_pack_weight(fwd, bwd, out_f, in_f, o, (int)(e - (int64_t)o * in_f), pe);
        }
    }
}

// checks + the block-prefix table -> a copy of the descriptor ready to launch
static int ao_plan(const sda_adamw_desc* dp, sda_adamw_desc* out) {
    if (!dp || dp->ntensor < 1 || dp->ntensor > SDA_ADAMW_MAXT) return SDA_E_BADARG;
    *out = *dp;
    int64_t blocks = 0;
    for (int t = 0; t < dp->ntensor; ++t) {
        if (!dp->p[t] || !dp->g[t] || !dp->m[t] || !dp->v[t] || dp->numel[t] < 1) return SDA_E_BADARG;
        const int kind = dp->pack_kind[t];
        if (kind < 0 || kind > 2) return SDA_E_BADARG;
        if (kind == 1) {
            const int o = dp->out_f[t], i = dp->in_f[t];
            if (o < 1 || i < 1 || o > 256 || i > 256) return SDA_E_UNSUPPORTED;
            if (dp->numel[t] != (int64_t)o * i || !dp->fwd[t] || !dp->bwd[t]) return SDA_E_BADARG;
        } else if (kind == 2) {
            if (dp->numel[t] > 256) return SDA_E_UNSUPPORTED;
            if (!dp->fwd[t]) return SDA_E_BADARG;
        }
        out->blk0[t] = (int)blocks;
        blocks += (dp->numel[t] + AO_CHUNK - 1) / AO_CHUNK;
        if (blocks > 0x7fffffffLL) return SDA_E_UNSUPPORTED;
    }
    for (int t = dp->ntensor; t <= SDA_ADAMW_MAXT; ++t) out->blk0[t] = (int)blocks;
    return SDA_OK;
}

static_assert(sizeof(sda_adamw_desc) <= 4096, "sda_adamw_desc travels by value: the kernel-argument segment holds 4096 bytes");

#ifndef SDA_HOST_EMU

__global__ __launch_bounds__(AO_THREADS) void adamw_step_kernel(const sda_adamw_desc d) {
    ao_thread(d, ao_step{d.decay, d.step_size, d.rsqrt_bc2}, blockIdx.x, threadIdx.x);
}

// the replayable form: the step's three scalars are row irow[0] of a device table (the caller keeps irow[0] inside the table)
__global__ __launch_bounds__(AO_THREADS) void adamw_dev_kernel(const sda_adamw_desc d, const float* __restrict__ table,
                                                               const int64_t* __restrict__ irow) {
    const float* row = table + 3 * irow[0];
    ao_thread(d, ao_step{row[0], row[1], row[2]}, blockIdx.x, threadIdx.x);
}

extern "C" int sda_adamw_step(const sda_adamw_desc* dp, void* stream) {
    sda_adamw_desc d;
    const int rc = ao_plan(dp, &d);
    if (rc != SDA_OK) return rc;
    hipLaunchKernelGGL(adamw_step_kernel, dim3((unsigned)d.blk0[d.ntensor]), dim3(AO_THREADS), 0, (hipStream_t)stream, d);
    return sda_launch_status();
}

extern "C" int sda_adamw_step_dev(const sda_adamw_desc* dp, const float* table, const int64_t* irow, void* stream) {
    if (!table || !irow) return SDA_E_BADARG;
    sda_adamw_desc d;
    const int rc = ao_plan(dp, &d);
    if (rc != SDA_OK) return rc;
    hipLaunchKernelGGL(adamw_dev_kernel, dim3((unsigned)d.blk0[d.ntensor]), dim3(AO_THREADS), 0, (hipStream_t)stream, d, table, irow);
    return sda_launch_status();
}

#else  // SDA_HOST_EMU: the CPU emulator (tests only; libsda_emu.so)

// Replays adamw_step_kernel on the host with HOST pointers: same checks, same block-prefix table, same per-thread function.
extern "C" int sda_adamw_step_emulate(const sda_adamw_desc* dp) {
    sda_adamw_desc d;
    const int rc = ao_plan(dp, &d);
    if (rc != SDA_OK) return rc;
    const ao_step s{d.decay, d.step_size, d.rsqrt_bc2};
    for (int b = 0; b < d.blk0[d.ntensor]; ++b)
        for (int tid = 0; tid < AO_THREADS; ++tid) ao_thread(d, s, b, tid);
    return SDA_OK;
}

// ... and adamw_dev_kernel: table and irow are HOST pointers too
extern "C" int sda_adamw_step_dev_emulate(const sda_adamw_desc* dp, const float* table, const int64_t* irow) {
    if (!table || !irow) return SDA_E_BADARG;
    sda_adamw_desc d;
    const int rc = ao_plan(dp, &d);
    if (rc != SDA_OK) return rc;
    const float* row = table + 3 * irow[0];
    const ao_step s{row[0], row[1], row[2]};
    for (int b = 0; b < d.blk0[d.ntensor]; ++b)
        for (int tid = 0; tid < AO_THREADS; ++tid) ao_thread(d, s, b, tid);
    return SDA_OK;
}
#endif
