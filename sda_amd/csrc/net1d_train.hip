// Parameter gradients of a whole single-level 1-D U-Net (the Lorenz GLOBAL score network of the reference's train_global; opt-in
// training, sda_amd/training.py with net1d = True).  A training step of that net on the per-layer kernels is ~47 launches around
// ~1 ms of kernel time: bound by launch latency and first-touch round trips, which is what csrc/net1d.hip removed from sampling.
// Here the step is one forward launch and THREE backward launches, whatever the depth, and one pack launch after the optimizer:
//   1. sda_net1d_fwd_train / sda_net1d_bwd_train: the kernels of net1d.hip (net1d.hpp, TRAIN = true: same tiles, same arithmetic,
//      the same outputs and saves bit for bit) that also write the tail's input, the cotangent at every convolution's output on the
//      own columns, and each tile's sums of the LayerNorm-backward term (the modulation rows' gradient) in a fixed slot;
//   2. sda_net1d_wgrad: ONE launch for all 2 + 2 nblocks convolutions.  Convolution v is an implicit GEMM dW[co][j] = sum_r G[r][co]
//      U[r][j] over the rows r = (image, position), with the columns j = 3 ci + tap in torch's (cin, 3) order and the bias as one more
//      column (U = 1) -- mlp_train.hip's discipline: the row axis is cut into `slabs` contiguous ranges (a function of the shapes only);
//      workgroup (slab, convolution, column tile) owns the 64 x 128 tile of one convolution's result over its slab and writes it,
//      unreduced, to work; per stage of 32 rows it stages G[32][64] and U[32][128] into LDS (U rebuilt from what the forward saved:
//      the strided net input, (a + mod - mean) rstd, act(z), the tail's input -- at position x + tap - 1, zero or wrapped beyond the
//      sequence; nothing is materialised), then each of the 4 waves issues v_mfma_f32_16x16x4_f32 over its 32 columns;
//   3. the slab reduction: sums the slabs in slab order (no atomics anywhere: bitwise reproducible), writes dW / db in torch's unpadded
//      layouts and finishes the modulation gradients from the per-tile sums (tile order, then image order for a shared row);
//   4. sda_net1d_pack: all weights and biases -> the forward buffer, the backward-data buffer and the padded bias rows of net1d.hip in
//      one launch (the bytes 2 x (2 + 2 nblocks) sda_pack_conv_weight launches and the bias copies produce: a pure permutation).
// Index arithmetic of 2 - 4 is in __host__ __device__ helpers; the emulators at the bottom (libsda_emu.so, tests only) replay the
// planner, the staging maps, the MFMA lane maps and the reduction order on the CPU.
#ifndef SDA_HOST_EMU
#include "net1d.hpp"
#else
#include "sda_common.hpp"
#endif

#define NW_MAXV (2 + 2 * SDA_NET1D_MAXB)   // convolutions of a net
#define NW_THREADS 256
#define NW_KP 32                 // rows per stage
#define NW_BM 64                 // output channels per workgroup: all of them (four 16-row MFMA tiles)
#define NW_BN 128                // columns per workgroup (4 waves x 2 x 16)
#define NW_MAX_SLABS 64
#define NW_TARGET_BLOCKS 1024    // enough workgroups to fill 256 CUs four times over
#define NW_ROW_G (NW_BM + 1)     // LDS row pitch (floats) of the staged cotangent
#define NW_ROW_U (NW_BN + 1)     // ... and of the staged input

struct NwGeom {
    int nconv;
    int slabs;
    int per;                              // rows per slab (a multiple of NW_KP)
    int tiles;                            // column tiles of all convolutions
    int grid;                             // tiles * slabs
    int elems;                            // sum of cout (3 cin + 1)
    int mod_rows;                         // rows of a block's modulation gradient: n (per image) or 1 (shared)
    int cin[NW_MAXV], cout[NW_MAXV];
    int tile0[NW_MAXV + 1];               // first tile of convolution v
    int elem0[NW_MAXV + 1];               // first element of convolution v in a slab of work: work[slab * elems + elem0[v] + o (3 cin + 1) + j]
};

__host__ __device__ inline int nw_ncol(int cin) { return 3 * cin + 1; }
__host__ __device__ inline int nw_n_colt(int cin) { return (nw_ncol(cin) + NW_BN - 1) / NW_BN; }

// need_bufs: a launch (or the replay) needs the operands and d->work; the planning entries size that buffer, so they do not ask for them
static int nw_plan(const sda_net1d_wgrad_desc* d, NwGeom* g, bool need_bufs) {
    if (!d) return SDA_E_BADARG;
    const sda_net1d_desc& t = d->net;
    if (t.n < 1 || t.len < 1 || t.c < 2 || t.c > 64 || t.cin < 1 || t.cin > 64 || t.cout < 1 || t.cout > 64 || t.nblocks < 0 ||
        t.nblocks > SDA_NET1D_MAXB)
        return SDA_E_UNSUPPORTED;
    if ((int64_t)t.len * 64 >= (1LL << 30) || (int64_t)t.n * t.len > 0x7fffffffLL) return SDA_E_UNSUPPORTED;
    if (t.x_sc < 0 || t.x_sx < 0 || d->gout_sc < 0 || d->gout_sx < 0) return SDA_E_UNSUPPORTED;
    if (d->slabs < 0 || d->slabs > NW_MAX_SLABS) return SDA_E_BADARG;
    if (need_bufs) {
        if (!d->work || !t.x || !d->gout || !d->g_save || !d->tail_in || d->g_stride < (int64_t)t.n * t.c * t.len) return SDA_E_BADARG;
        if (t.nblocks > 0 && (!t.a_save || !t.z_save || !t.mean_save || !t.rstd_save || !d->mod_part || d->mod_tiles < 1)) return SDA_E_BADARG;
    }
    g->nconv = 2 + 2 * t.nblocks;
    g->tile0[0] = 0; g->elem0[0] = 0;
    for (int v = 0; v < g->nconv; ++v) {
        g->cin[v] = v == 0 ? t.cin : t.c;
        g->cout[v] = v == g->nconv - 1 ? t.cout : t.c;
        g->tile0[v + 1] = g->tile0[v] + nw_n_colt(g->cin[v]);
        g->elem0[v + 1] = g->elem0[v] + g->cout[v] * nw_ncol(g->cin[v]);
    }
    g->tiles = g->tile0[g->nconv];
    g->elems = g->elem0[g->nconv];
    g->mod_rows = t.mod_sn != 0 ? t.n : 1;
    const int rows = t.n * t.len;
    const int stages = (rows + NW_KP - 1) / NW_KP;
    int s = d->slabs;
    if (s == 0) {                                            // the planner's choice: a function of the shapes only
        s = (NW_TARGET_BLOCKS + g->tiles - 1) / g->tiles;
        if (s > NW_MAX_SLABS) s = NW_MAX_SLABS;
    }
    if (s > stages) s = stages;
    if (s < 1) s = 1;
    g->per = (stages + s - 1) / s * NW_KP;
    g->slabs = (rows + g->per - 1) / g->per;                 // (no empty slab)
    g->grid = g->tiles * g->slabs;
    return SDA_OK;
}

// ---------------------------------------------------------------- index helpers (host + device)

// workgroup b -> (slab, convolution, column tile)
__host__ __device__ inline void nw_decode_block(const NwGeom& g, int b, int& slab, int& conv, int& colt) {
    slab = b / g.tiles;
    const int t = b - slab * g.tiles;
    conv = 0;
    while (conv + 1 < g.nconv && t >= g.tile0[conv + 1]) ++conv;
    colt = t - g.tile0[conv];
}

// staging maps: element e of a stage's G tile [NW_KP rows][NW_BM channels] / U tile [NW_KP rows][NW_BN columns] -> (row of the stage,
// column); thread tid stages elements tid + NW_THREADS i.  G: consecutive threads read consecutive POSITIONS of a channel plane, and so
// does U up to the tap shift (the operands are planar [channel][position])
__host__ __device__ inline void nw_stage_g(int e, int& r, int& col) { col = e / NW_KP; r = e - col * NW_KP; }
__host__ __device__ inline void nw_stage_u(int e, int& r, int& col) { col = e / NW_KP; r = e - col * NW_KP; }

// the cotangent at output channel o of convolution v, image n, position x
__host__ __device__ inline float nw_load_g(const sda_net1d_wgrad_desc& d, const NwGeom& g, int v, int n, int x, int o) {
    if (o >= g.cout[v]) return 0.f;
    const sda_net1d_desc& t = d.net;
    if (v == g.nconv - 1) return d.gout[(int64_t)n * d.gout_sn + (int64_t)o * d.gout_sc + (int64_t)x * d.gout_sx];
    const int slot = v == 0 ? 2 * t.nblocks : ((v - 1) & 1) ? v - 2 : v;          // conv1 of block k (v = 1 + 2 k): 2 k + 1; conv2 (v = 2 + 2 k): 2 k
    return d.g_save[(int64_t)slot * d.g_stride + ((int64_t)n * t.c + o) * t.len + x];
}

// column j of the multiply's second operand at (image n, position x): U[ci][x + tap - 1] for j = 3 ci + tap < 3 cin (zero, or wrapped,
// beyond the sequence), the constant 1 (the bias column) for j == 3 cin, 0 beyond
__host__ __device__ inline float nw_load_u(const sda_net1d_wgrad_desc& d, const NwGeom& g, int v, int n, int x, int j) {
    const sda_net1d_desc& t = d.net;
    const int cin = g.cin[v];
    if (j >= 3 * cin) return j == 3 * cin ? 1.f : 0.f;
    const int ci = j / 3, tap = j - 3 * ci;
    int p = x + tap - 1;
    if (p < 0 || p >= t.len) {
        if (!t.circular) return 0.f;
        p = p < 0 ? p + t.len : p - t.len;
    }
    if (v == 0) return t.x[(int64_t)n * t.x_sn + (int64_t)ci * t.x_sc + (int64_t)p * t.x_sx];
    if (v == g.nconv - 1) return d.tail_in[((int64_t)n * t.c + ci) * t.len + p];
    const int k = (v - 1) >> 1;
    const int64_t e = (int64_t)k * t.save_stride + ((int64_t)n * t.c + ci) * t.len + p;
    if ((v - 1) & 1) return sda_act(t.act, t.z_save[e]);                           // conv2: act(z)
    const int64_t s = (int64_t)k * t.stat_stride + (int64_t)n * t.len + p;
    const float mo = t.mod[k] ? t.mod[k][(int64_t)n * t.mod_sn + ci] : 0.f;
    return (t.a_save[e] + mo - t.mean_save[s]) * t.rstd_save[s];                    // conv1: the forward's order, (a + mod) - mean, then x rstd
}

// reduction of element e: e < elems: one weight / bias gradient over the slabs, in slab order; beyond: one modulation gradient
// (block k, row i, channel ch) over the tiles in tile order -- and, for a shared row, over the images in image order
__host__ __device__ inline void nw_reduce_one(const sda_net1d_wgrad_desc& d, const NwGeom& g, int e) {
    const sda_net1d_desc& t = d.net;
    if (e < g.elems) {
        float s = 0.f;
        for (int k = 0; k < g.slabs; ++k) s += d.work[(int64_t)k * g.elems + e];
        int v = 0;
        while (v + 1 < g.nconv && e >= g.elem0[v + 1]) ++v;
        const int local = e - g.elem0[v], ncol = nw_ncol(g.cin[v]);
        const int o = local / ncol, j = local - o * ncol;
        if (j < ncol - 1) { if (d.dw[v]) d.dw[v][(int64_t)o * (ncol - 1) + j] = s; }
        else if (d.db[v]) d.db[v][o] = s;
        return;
    }
    int m = e - g.elems;
    const int ch = m % t.c;
    m /= t.c;
    const int i = m % g.mod_rows, k = m / g.mod_rows;
    if (k >= t.nblocks || !d.dmod[k]) return;
    const float* part = d.mod_part + (int64_t)k * t.n * d.mod_tiles * t.c + ch;
    float s = 0.f;
    if (t.mod_sn != 0) {
        for (int tl = 0; tl < d.mod_tiles; ++tl) s += part[((int64_t)i * d.mod_tiles + tl) * t.c];
        d.dmod[k][(int64_t)i * d.dmod_sn + ch] = s;
    } else {
        for (int64_t q = 0; q < (int64_t)t.n * d.mod_tiles; ++q) s += part[q * t.c];
        d.dmod[k][ch] = s;
    }
}
__host__ __device__ inline int nw_reduce_elems(const sda_net1d_wgrad_desc& d, const NwGeom& g) {
    return g.elems + d.net.nblocks * g.mod_rows * d.net.c;
}

// ---------------------------------------------------------------- pack: index helpers (host + device)
#define NP_SLAB (3 * 64 * 64)
__host__ __device__ inline int np_cin(const sda_net1d_pack_desc& p, int v) { return v == 0 ? p.cin : p.c; }
__host__ __device__ inline int np_cout(const sda_net1d_pack_desc& p, int v) { return v == 1 + 2 * p.nblocks ? p.cout : p.c; }
// element i of the forward buffer: slab v = forward convolution v, [tap][ci][co]
__host__ __device__ inline float np_fwd(const sda_net1d_pack_desc& p, int i) {
    const int v = i / NP_SLAB, e = i - v * NP_SLAB, tap = e >> 12, ci = (e >> 6) & 63, co = e & 63;
    const int cin = np_cin(p, v), cout = np_cout(p, v);
    return (ci < cin && co < cout) ? p.w[v][(co * cin + ci) * 3 + tap] : 0.f;
}
// element i of the backward-data buffer: slab s in execution order (tail^T, (conv2^T, conv1^T) of block nblocks - 1 .. 0, head^T),
// [tap][co][ci] with the taps reversed; head^T keeps cin_keep input channels
__host__ __device__ inline float np_bwd(const sda_net1d_pack_desc& p, int i) {
    const int nconv = 2 + 2 * p.nblocks;
    const int s = i / NP_SLAB, e = i - s * NP_SLAB, tap = e >> 12, co = (e >> 6) & 63, ci = e & 63;
    const int v = nconv - 1 - s;                             // (execution order of the VJP = the forward's, reversed)
    const int cin = np_cin(p, v), cout = np_cout(p, v);
    const int keep = v == 0 ? p.cin_keep : cin;
    return (ci < keep && ci < cin && co < cout) ? p.w[v][(co * cin + ci) * 3 + (2 - tap)] : 0.f;
}
__host__ __device__ inline float np_bias(const sda_net1d_pack_desc& p, int i) {
    const int v = i >> 6, o = i & 63;
    return (p.b[v] && o < np_cout(p, v)) ? p.b[v][o] : 0.f;
}
static int np_check(const sda_net1d_pack_desc* p) {
    if (!p) return SDA_E_BADARG;
    if (p->nblocks < 0 || p->nblocks > SDA_NET1D_MAXB || p->c < 2 || p->c > 64 || p->cin < 1 || p->cin > 64 || p->cout < 1 || p->cout > 64)
        return SDA_E_UNSUPPORTED;
    if (p->cin_keep < 0) return SDA_E_BADARG;
    for (int v = 0; v < 2 + 2 * p->nblocks; ++v)
        if (!p->w[v]) return SDA_E_BADARG;
    return SDA_OK;
}

// ------------------------------------------------------------------------------------------------------------ the kernels
#ifndef SDA_HOST_EMU

__global__ __launch_bounds__(NW_THREADS) void net1d_wgrad_kernel(const sda_net1d_wgrad_desc d, const NwGeom g) {
    constexpr int MT = NW_BM / 16, NT = NW_BN / 64;          // 16 x 16 tiles per wave: 4 down the channels, 2 across its 32 columns
    __shared__ float s_g[NW_KP * NW_ROW_G];
    __shared__ float s_u[NW_KP * NW_ROW_U];
    __shared__ int s_n[NW_KP], s_x[NW_KP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;
    int slab, conv, colt;
    nw_decode_block(g, blockIdx.x, slab, conv, colt);
    const int col0 = colt * NW_BN;
    const int cout = g.cout[conv], ncol = nw_ncol(g.cin[conv]);
    const int len = d.net.len, rows = d.net.n * len;

    n1_f32x4 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[m][nt] = n1_f32x4{0.f, 0.f, 0.f, 0.f};

    const int r_begin = slab * g.per;
    const int r_end = r_begin + g.per < rows ? r_begin + g.per : rows;
    for (int r0 = r_begin; r0 < r_end; r0 += NW_KP) {
        if (tid < NW_KP) {                                   // (image, position) of the stage's rows: one division per row, not per element
            const int row = r0 + tid < r_end ? r0 + tid : r_end - 1;
            const int n = row / len;
            s_n[tid] = n; s_x[tid] = row - n * len;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NW_KP * NW_BM / NW_THREADS; ++i) {
            int r, col;
            nw_stage_g(tid + NW_THREADS * i, r, col);
            s_g[r * NW_ROW_G + col] = r0 + r < r_end ? nw_load_g(d, g, conv, s_n[r], s_x[r], col) : 0.f;
        }
#pragma unroll
        for (int i = 0; i < NW_KP * NW_BN / NW_THREADS; ++i) {
            int r, col;
            nw_stage_u(tid + NW_THREADS * i, r, col);
            s_u[r * NW_ROW_U + col] = r0 + r < r_end ? nw_load_u(d, g, conv, s_n[r], s_x[r], col0 + col) : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k4 = 0; k4 < NW_KP / 4; ++k4) {
            const int kk = 4 * k4 + kq;
            float b[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b[nt] = s_u[kk * NW_ROW_U + wave * 32 + nt * 16 + li];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const float a = s_g[kk * NW_ROW_G + m * 16 + li];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[nt], acc[m][nt], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    float* out = d.work + (int64_t)slab * g.elems + g.elem0[conv];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int j = col0 + wave * 32 + nt * 16 + li;
        if (j >= ncol) continue;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = m * 16 + 4 * kq + r;
                if (o < cout) out[(int64_t)o * ncol + j] = acc[m][nt][r];
            }
    }
}

__global__ __launch_bounds__(256) void net1d_wgrad_reduce_kernel(const sda_net1d_wgrad_desc d, const NwGeom g) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < nw_reduce_elems(d, g)) nw_reduce_one(d, g, e);
}

extern "C" int sda_net1d_wgrad(const sda_net1d_wgrad_desc* d, void* stream) {
    NwGeom g;
    const int rc = nw_plan(d, &g, true);
    if (rc != SDA_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(net1d_wgrad_kernel, dim3(g.grid), dim3(NW_THREADS), 0, st, *d, g);
    const int lr = sda_launch_status();
    if (lr != SDA_OK) return lr;
    hipLaunchKernelGGL(net1d_wgrad_reduce_kernel, dim3((nw_reduce_elems(*d, g) + 255) / 256), dim3(256), 0, st, *d, g);
    return sda_launch_status();
}

__global__ __launch_bounds__(256) void net1d_pack_kernel(const sda_net1d_pack_desc p) {
    const int total = (2 + 2 * p.nblocks) * NP_SLAB;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        if (p.wf) p.wf[i] = np_fwd(p, i);
        if (p.wb) p.wb[i] = np_bwd(p, i);
        if (p.bias && i < (2 + 2 * p.nblocks) * 64) p.bias[i] = np_bias(p, i);
    }
}

extern "C" int sda_net1d_pack(const sda_net1d_pack_desc* p, void* stream) {
    const int rc = np_check(p);
    if (rc != SDA_OK) return rc;
    const int total = (2 + 2 * p->nblocks) * NP_SLAB;
    hipLaunchKernelGGL(net1d_pack_kernel, dim3((total + 1023) / 1024), dim3(256), 0, (hipStream_t)stream, *p);
    return sda_launch_status();
}

// ------------------------------------------------------------------------------------------------------------ forward / VJP with saves
template <bool BWD, int NF>
static void net1d_train_launch_nf(const sda_net1d_desc& d, const N1Train& t, dim3 grid, int ptiles, int tp, int whole, hipStream_t stream) {
    if (BWD) hipLaunchKernelGGL((net1d_bwd_kernel<NF, false, true>), grid, dim3(256), 0, stream, d, t, ptiles, tp, whole);
    else hipLaunchKernelGGL((net1d_fwd_kernel<NF, false, true>), grid, dim3(256), 0, stream, d, t, ptiles, tp, whole);
}

template <bool BWD>
static int net1d_train_launch(const sda_net1d_train_desc* td, hipStream_t stream) {
    if (!td) return SDA_E_BADARG;
    const sda_net1d_desc* d = &td->net;
    const int rc = net1d_check(d, BWD);
    if (rc != SDA_OK) return rc;
    int tp, ptiles, whole;
    const int nf = net1d_tiling(d, &tp, &ptiles, &whole);
    if (!nf) return SDA_E_UNSUPPORTED;
    if ((int64_t)d->n * ptiles > 0x7fffffffLL) return SDA_E_UNSUPPORTED;
    if (!BWD) {
        if (!td->tail_in || (d->nblocks > 0 && !d->a_save)) return SDA_E_BADARG;
    } else {
        if (!td->g_save || td->g_stride < (int64_t)d->n * d->c * d->len) return SDA_E_BADARG;
        if (d->nblocks > 0 && (!td->mod_part || td->mod_tiles != ptiles)) return SDA_E_BADARG;
    }
    const N1Train t = {td->tail_in, td->g_save, td->g_stride, td->mod_part};
    const dim3 grid((unsigned)(d->n * ptiles));
    switch (nf) {
        case 2: net1d_train_launch_nf<BWD, 2>(*d, t, grid, ptiles, tp, whole, stream); break;
        case 3: net1d_train_launch_nf<BWD, 3>(*d, t, grid, ptiles, tp, whole, stream); break;
        case 4: net1d_train_launch_nf<BWD, 4>(*d, t, grid, ptiles, tp, whole, stream); break;
        default: net1d_train_launch_nf<BWD, 5>(*d, t, grid, ptiles, tp, whole, stream); break;
    }
    return sda_launch_status();
}

extern "C" int sda_net1d_fwd_train(const sda_net1d_train_desc* t, void* stream) { return net1d_train_launch<false>(t, (hipStream_t)stream); }
extern "C" int sda_net1d_bwd_train(const sda_net1d_train_desc* t, void* stream) { return net1d_train_launch<true>(t, (hipStream_t)stream); }

#endif  // !SDA_HOST_EMU

// planning entries (host only: nothing is launched)
extern "C" int sda_net1d_wgrad_slabs(const sda_net1d_wgrad_desc* d) {
    NwGeom g;
    const int rc = nw_plan(d, &g, false);
    return rc != SDA_OK ? rc : g.slabs;
}

extern "C" int64_t sda_net1d_wgrad_work_floats(const sda_net1d_wgrad_desc* d) {
    NwGeom g;
    const int rc = nw_plan(d, &g, false);
    return rc != SDA_OK ? (int64_t)rc : (int64_t)g.slabs * g.elems;
}

// ------------------------------------------------------------------------------------------------------------ CPU emulators (tests only; libsda_emu.so)
#ifdef SDA_HOST_EMU
#include <algorithm>
#include <vector>
// Replays net1d_wgrad_kernel + net1d_wgrad_reduce_kernel on the host with HOST pointers (d->work included): same planner, same block
// decode, same staging maps, same MFMA lane maps (v_mfma_f32_16x16x4_f32: A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15], D row =
// 4 (l >> 4) + r, col = l & 15) in the same k order, same slab-ordered reduction.
extern "C" int sda_net1d_wgrad_emulate(const sda_net1d_wgrad_desc* dp) {
    NwGeom g;
    const int rc = nw_plan(dp, &g, true);
    if (rc != SDA_OK) return rc;
    const sda_net1d_wgrad_desc& d = *dp;
    constexpr int MT = NW_BM / 16, NT = NW_BN / 64;
    std::vector<float> s_g((size_t)NW_KP * NW_ROW_G), s_u((size_t)NW_KP * NW_ROW_U), acc((size_t)NW_THREADS * MT * NT * 4);
    int s_n[NW_KP], s_x[NW_KP];
    const int len = d.net.len, rows = d.net.n * len;
    for (int b = 0; b < g.grid; ++b) {
        int slab, conv, colt;
        nw_decode_block(g, b, slab, conv, colt);
        const int col0 = colt * NW_BN;
        const int cout = g.cout[conv], ncol = nw_ncol(g.cin[conv]);
        std::fill(acc.begin(), acc.end(), 0.f);
        const int r_begin = slab * g.per;
        const int r_end = r_begin + g.per < rows ? r_begin + g.per : rows;
        for (int r0 = r_begin; r0 < r_end; r0 += NW_KP) {
            for (int tid = 0; tid < NW_KP; ++tid) {
                const int row = r0 + tid < r_end ? r0 + tid : r_end - 1;
                s_n[tid] = row / len; s_x[tid] = row - s_n[tid] * len;
            }
            for (int tid = 0; tid < NW_THREADS; ++tid) {
                for (int i = 0; i < NW_KP * NW_BM / NW_THREADS; ++i) {
                    int r, col;
                    nw_stage_g(tid + NW_THREADS * i, r, col);
                    s_g[(size_t)r * NW_ROW_G + col] = r0 + r < r_end ? nw_load_g(d, g, conv, s_n[r], s_x[r], col) : 0.f;
                }
                for (int i = 0; i < NW_KP * NW_BN / NW_THREADS; ++i) {
                    int r, col;
                    nw_stage_u(tid + NW_THREADS * i, r, col);
                    s_u[(size_t)r * NW_ROW_U + col] = r0 + r < r_end ? nw_load_u(d, g, conv, s_n[r], s_x[r], col0 + col) : 0.f;
                }
            }
            for (int wave = 0; wave < 4; ++wave)
                for (int k4 = 0; k4 < NW_KP / 4; ++k4)
                    for (int m = 0; m < MT; ++m)
                        for (int nt = 0; nt < NT; ++nt) {
                            float A[16][4], B[4][16];
                            for (int lane = 0; lane < 64; ++lane) {
                                const int li = lane & 15, kq = lane >> 4, kk = 4 * k4 + kq;
                                B[kq][li] = s_u[(size_t)kk * NW_ROW_U + wave * 32 + nt * 16 + li];
                                A[li][kq] = s_g[(size_t)kk * NW_ROW_G + m * 16 + li];
                            }
                            for (int lane = 0; lane < 64; ++lane)
                                for (int r = 0; r < 4; ++r) {
                                    const int i = 4 * (lane >> 4) + r, jj = lane & 15;
                                    float& cv = acc[(((size_t)(wave * 64 + lane) * MT + m) * NT + nt) * 4 + r];
                                    for (int k = 0; k < 4; ++k) cv = fmaf(A[i][k], B[k][jj], cv);
                                }
                        }
        }
        for (int tid = 0; tid < NW_THREADS; ++tid) {
            const int lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;
            for (int nt = 0; nt < NT; ++nt) {
                const int j = col0 + wave * 32 + nt * 16 + li;
                if (j >= ncol) continue;
                for (int m = 0; m < MT; ++m)
                    for (int r = 0; r < 4; ++r) {
                        const int o = m * 16 + 4 * kq + r;
                        if (o < cout) d.work[(int64_t)slab * g.elems + g.elem0[conv] + (int64_t)o * ncol + j] = acc[(((size_t)tid * MT + m) * NT + nt) * 4 + r];
                    }
            }
        }
    }
    const int ne = nw_reduce_elems(d, g);
    for (int e = 0; e < ne; ++e) nw_reduce_one(d, g, e);
    return SDA_OK;
}

// Replays net1d_pack_kernel on the host with HOST pointers.
extern "C" int sda_net1d_pack_emulate(const sda_net1d_pack_desc* pp) {
    const int rc = np_check(pp);
    if (rc != SDA_OK) return rc;
    const sda_net1d_pack_desc& p = *pp;
    const int total = (2 + 2 * p.nblocks) * NP_SLAB;
    for (int i = 0; i < total; ++i) {
        if (p.wf) p.wf[i] = np_fwd(p, i);
        if (p.wb) p.wb[i] = np_bwd(p, i);
        if (p.bias && i < (2 + 2 * p.nblocks) * 64) p.bias[i] = np_bias(p, i);
    }
    return SDA_OK;
}
#endif  // SDA_HOST_EMU
