// Weight gradient of the 3 x 3, stride-1 block convolutions: the tiled route beside the general kernel (conv_wgrad.hip).
//
//   dW[co][ci][ky][kx] = sum_{n,oy,ox} g[n][co][oy][ox] * V(n, ci, oy + ky - 1, ox + kx - 1),   db[co] = sum g
//
// Served (sda_conv_wgrad3_serves): 2-D, kh = kw = 3, stride 1, no up-sampling / zero insertion / pooling, no context channels, no
// explicit pad, planar contiguous source, cx % 32 == 0, cout % 32 == 0, circular or zero padding, loader = LayerNorm + modulation
// (conv1), activation (conv2) or none.  Everything else: SDA_E_UNSUPPORTED (the general kernel serves it).
//
// Design:
//   * a stage is R output rows of one image, all W columns.  The workgroup (4 waves) stages the input rows y0-1 .. y0+R of its 32
//     channels ONCE, halo included, as V[32][(R+2) x (W+2)] (wrap / zero padding and the loader's LayerNorm / modulation /
//     activation applied here, through the general kernel's own loader helper), and the cotangent as g[BM][R x (W+2)] with the two
//     pad columns of every row zero: both tiles then share one position index q = r (W+2) + ox, and the B operand of tap (ky, kx)
//     is the V tile read at q + ky (W+2) + kx -- nine shifted reads of one tile instead of nine staged copies;
//   * v_mfma_f32_16x16x4_f32 with M = cout, N = cin, K = positions: A = g[co = lane&15][q = 4 ks + (lane>>4)], B = V[ci = lane&15][...],
//     D row = wg3_mfma_row(r, lane), col = lane&15.  Wave w owns the 16-channel half (w & 1) of the 32 input channels and the MT
//     16-cout tiles (w >> 1) MT ..: its g fragments are loaded once per K step and reused for all nine taps, and its 9 x MT
//     accumulator tiles (108 VGPRs at the 96-cout tile) stay in registers for the whole slab;
//   * the workgroups of the first cin tile also multiply g by a column of ones: db;
//   * LDS channel pitches are = 2 (mod 32) floats: the 16 channels x 2 positions a 32-lane half reads with ds_read_b32 fall on 32
//     different banks, whatever the tap shift;
//   * the position axis (stages) is cut into slabs; a workgroup writes its tile, unreduced, to work[slab][co][ci*9 + tap] -- the
//     general kernel's column order, ones column last -- and the general kernel's slab-order reduction finishes: no atomics,
//     bitwise reproducible, `accumulate` as there.
//
// Index arithmetic is in __host__ __device__ helpers; the emulator at the bottom (libsda_emu.so, tests only) replays the planner,
// the staging walk and maps (halo, wrap, zero pad), the tap offsets, the MFMA lane maps and the reduction order on the CPU.
#include "conv_wgrad3.hpp"

// -> SDA_OK and the plan, SDA_E_UNSUPPORTED outside the served set, SDA_E_BADARG as the general planner
static int wg3_plan(const sda_wgrad_desc* wd, Wg3Geom* t, WgradGeom* g) {
    if (!wd) return SDA_E_BADARG;
    sda_wgrad_desc chk = *wd;
    chk.slabs = 0;                                            // (this route has its own slab range)
    int rc = wgrad_plan(&chk, g);
    if (rc != SDA_OK) return rc;
    const sda_conv_desc& d = wd->conv;
    if (wd->slabs < 0 || wd->slabs > WG3_MAX_SLABS) return SDA_E_BADARG;
    if (d.kh != 3 || d.kw != 3 || d.stride_h != 1 || d.stride_w != 1 || d.up_h != 1 || d.up_w != 1) return SDA_E_UNSUPPORTED;
    if (d.cctx > 0 || d.explicit_pad) return SDA_E_UNSUPPORTED;
    if (d.x_sx != 1 || d.x_sy != d.ws || d.x_sc != (int64_t)d.hs * d.ws || d.n_inner != 1) return SDA_E_UNSUPPORTED;
    if (d.cx % WG3_CI || d.cout % 32) return SDA_E_UNSUPPORTED;
    if (d.ho != d.hs || d.wo != d.ws) return SDA_E_UNSUPPORTED;
    const bool ln = d.ln_mean != nullptr, mod = d.mod != nullptr, act = d.act_in != 0;
    if (!((ln && mod && !act) || (!ln && !mod))) return SDA_E_UNSUPPORTED;     // conv1 | conv2 or plain
    t->H = d.hs;
    t->W = d.ws;
    t->W2 = d.ws + 2;
    if (t->W2 > 4096) return SDA_E_UNSUPPORTED;
    int R = WG3_Q / t->W2;
    if (R < 1) R = 1;
    if (R > t->H) R = t->H;
    t->R = R;
    t->nrb = (t->H + R - 1) / R;
    const int64_t S = (int64_t)d.n * t->nrb;
    if (S > 0x7fffffffL) return SDA_E_UNSUPPORTED;
    t->S = (int)S;
    t->mt = d.cout % 96 == 0 ? 3 : d.cout % 64 == 0 ? 2 : 1;
    t->bm = 32 * t->mt;
    t->n_ct = d.cout / t->bm;
    t->n_cit = d.cx / WG3_CI;
    t->q4 = (R * t->W2 + 3) / 4 * 4;
    t->gp = wg3_pitch(t->q4);
    t->vp = wg3_pitch(t->q4 + 2 * t->W2 + 2);                 // (the last K step of tap (2, 2) reads up to q4 - 1 + 2 W2 + 2)
    const int64_t lds = 4 * ((int64_t)WG3_CI * t->vp + (int64_t)t->bm * t->gp);
    if (lds > WG3_LDS_MAX) return SDA_E_UNSUPPORTED;
    t->lds_bytes = (int)lds;
    const int64_t tiles = (int64_t)t->n_ct * t->n_cit;
    int64_t s = wd->slabs;
    if (s == 0) {                                             // the planner's choice: a function of the shape only
        s = WG3_TARGET_BLOCKS / tiles;
        if (s > WG3_MAX_SLABS) s = WG3_MAX_SLABS;
    }
    if (s > S) s = S;
    if (s < 1) s = 1;
    t->per = (int)((S + s - 1) / s);
    t->slabs = (int)((S + t->per - 1) / t->per);              // (no empty slab)
    if (tiles * t->slabs > 0x7fffffffL) return SDA_E_UNSUPPORTED;
    t->grid = (int)(tiles * t->slabs);
    g->slabs = t->slabs;                                      // what the shared reduction reads
    return SDA_OK;
}

// element (row, col) of channel ci of the staged input tile of stage (n, y0): V(n, ci, y0 - 1 + row, col - 1), wrapped or zero-padded
__host__ __device__ inline float wg3_stage_v(const sda_conv_desc& d, const Wg3Geom& t, int n, int y0, int ci, int row, int col) {
    int y = y0 - 1 + row, x = col - 1;                        // y in [-1, H + R), x in [-1, W]
    if (d.circular) {
        if (y < 0) y += t.H;
        if (y >= t.H) y -= t.H;                               // (R <= H: once is enough)
        if (x < 0) x += t.W;
        if (x >= t.W) x -= t.W;
    } else if (y < 0 || y >= t.H || x < 0 || x >= t.W) {
        return 0.f;
    }
    return wgrad_load_src(d, n, ci, y, x);
}

// LDS offset of tap (ky, kx) relative to the position index
__host__ __device__ inline int wg3_tap_offset(const Wg3Geom& t, int tap) {
    const int ky = tap / 3;
    return ky * t.W2 + (tap - 3 * ky);
}

// ---------------------------------------------------------------- the kernel
#ifndef SDA_HOST_EMU

typedef float wg3_f32x4 __attribute__((ext_vector_type(4)));

template <int MT>
__global__ __launch_bounds__(WG3_THREADS, 2) void conv_wgrad3_kernel(const sda_wgrad_desc wd, const Wg3Geom t, const int ncol) {
    constexpr int BM = 32 * MT;
    extern __shared__ __attribute__((aligned(16))) float wg3_lds[];
    float* const s_v = wg3_lds;                               // [32][vp]
    float* const s_g = wg3_lds + WG3_CI * t.vp;               // [BM][gp]
    sda_conv_desc d = wd.conv;
    d.n_inner = 1;                                            // the served set, spelled out for the loader helper's arithmetic
    d.x_sx = 1;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int l15 = lane & 15;
    const int kq = lane >> 4;
    int slab, ct, cit;
    wg3_decode_block(t, blockIdx.x, slab, ct, cit);
    const int co0 = ct * BM;
    const int ci0 = cit * WG3_CI;
    const bool bias = cit == 0;
    const int chalf = wave & 1;                               // this wave's 16 input channels
    const int cot0 = (wave >> 1) * MT;                        // ... and its first 16-cout tile

    // the pad tails of both tiles are never staged: zero everything once
    for (int i = tid; i < WG3_CI * t.vp + BM * t.gp; i += WG3_THREADS) wg3_lds[i] = 0.f;

    wg3_f32x4 acc[9][MT];
    wg3_f32x4 accb[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) acc[tap][m] = (wg3_f32x4){0.f, 0.f, 0.f, 0.f};
        accb[m] = (wg3_f32x4){0.f, 0.f, 0.f, 0.f};
    }
    int off[9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) off[tap] = wg3_tap_offset(t, tap);

    const float* const vb = s_v + (chalf * 16 + l15) * t.vp + kq;
    const float* const gb = s_g + (cot0 * 16 + l15) * t.gp + kq;
    const Wg3Walk wv0 = wg3_walk_begin(tid, t.W2, t.R + 2);
    const Wg3Walk wg0 = wg3_walk_begin(tid, t.W2, t.R);

    const int s_begin = slab * t.per;
    const int s_end = s_begin + t.per < t.S ? s_begin + t.per : t.S;
    for (int s = s_begin; s < s_end; ++s) {
        const int n = s / t.nrb;
        const int y0 = (s - n * t.nrb) * t.R;
        __syncthreads();                                      // the previous stage's reads (and the clear) are done
        for (Wg3Walk w = wv0; w.ch < WG3_CI; wg3_walk_next(w))
            s_v[w.ch * t.vp + w.row * t.W2 + w.col] = wg3_stage_v(d, t, n, y0, ci0 + w.ch, w.row, w.col);
        for (Wg3Walk w = wg0; w.ch < BM; wg3_walk_next(w))
            s_g[w.ch * t.gp + w.row * t.W2 + w.col] = wg3_stage_g(wd, t, n, y0, co0 + w.ch, w.row, w.col);
        __syncthreads();
        for (int q = 0; q < t.q4; q += 4) {
            float a[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m) a[m] = gb[m * 16 * t.gp + q];
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const float b = vb[q + off[tap]];
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[tap][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], b, acc[tap][m], 0, 0, 0);
            }
            if (bias && chalf == 0) {
#pragma unroll
                for (int m = 0; m < MT; ++m) accb[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], 1.f, accb[m], 0, 0, 0);
            }
        }
    }

    float* const out = wd.work + (int64_t)slab * d.cout * ncol;
    const int ci = ci0 + chalf * 16 + l15;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = co0 + (cot0 + m) * 16 + wg3_mfma_row(r, lane);
            float* const o = out + (int64_t)co * ncol;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) o[ci * 9 + tap] = acc[tap][m][r];
            if (bias && chalf == 0 && l15 == 0) o[ncol - 1] = accb[m][r];
        }
}

template <int MT>
static int wg3_launch_t(const sda_wgrad_desc* d, const Wg3Geom& t, const WgradGeom& g, hipStream_t stream) {
    static bool raised[SDA_MAX_DEVICES];
    int rc = sda_raise_dyn_lds((const void*)conv_wgrad3_kernel<MT>, WG3_LDS_MAX, raised);
    if (rc != SDA_OK) return rc;
    hipLaunchKernelGGL(conv_wgrad3_kernel<MT>, dim3(t.grid), dim3(WG3_THREADS), t.lds_bytes, stream, *d, t, g.ncol);
    return sda_launch_status();
}

extern "C" int sda_conv_wgrad3(const sda_wgrad_desc* d, void* stream) {
    Wg3Geom t;
    WgradGeom g;
    int rc = wg3_plan(d, &t, &g);
    if (rc != SDA_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    switch (t.mt) {
        case 1: rc = wg3_launch_t<1>(d, t, g, st); break;
        case 2: rc = wg3_launch_t<2>(d, t, g, st); break;
        default: rc = wg3_launch_t<3>(d, t, g, st); break;
    }
    if (rc != SDA_OK) return rc;
    return wgrad_launch_reduce(d, g, st);
}

#endif  // !SDA_HOST_EMU

// planning entries (host only: nothing is launched)
extern "C" int sda_conv_wgrad3_serves(const sda_wgrad_desc* d) {
    Wg3Geom t;
    WgradGeom g;
    return wg3_plan(d, &t, &g) == SDA_OK ? 1 : 0;
}

extern "C" int64_t sda_conv_wgrad3_work_floats(const sda_wgrad_desc* d) {
    Wg3Geom t;
    WgradGeom g;
    int rc = wg3_plan(d, &t, &g);
    return rc != SDA_OK ? (int64_t)rc : (int64_t)t.slabs * d->conv.cout * g.ncol;
}

// ---------------------------------------------------------------- CPU emulator (tests only; libsda_emu.so)
#ifdef SDA_HOST_EMU
#include <vector>
extern "C" int sda_conv_wgrad3_slabs(const sda_wgrad_desc* d) {
    Wg3Geom t;
    WgradGeom g;
    int rc = wg3_plan(d, &t, &g);
    return rc != SDA_OK ? rc : t.slabs;
}

// Replays conv_wgrad3_kernel<MT> + the shared slab reduction on the host with HOST pointers (d->work included): same planner, same
// staging walk and element maps, same tap offsets, same MFMA lane maps (A[i = l&15][k = l>>4], B[k = l>>4][j = l&15], D row =
// wg3_mfma_row(r, l), col = l&15) in the same K order.  Reads outside the LDS image abort the replay with SDA_E_LDS.
extern "C" int sda_conv_wgrad3_emulate(const sda_wgrad_desc* dp) {
    Wg3Geom t;
    WgradGeom g;
    int rc = wg3_plan(dp, &t, &g);
    if (rc != SDA_OK) return rc;
    const sda_wgrad_desc& wd = *dp;
    const sda_conv_desc& d = wd.conv;
    const int MT = t.mt, BM = t.bm;
    const size_t nv = (size_t)WG3_CI * t.vp, ng = (size_t)BM * t.gp;
    if ((int)(4 * (nv + ng)) != t.lds_bytes) return SDA_E_LDS;
    std::vector<float> lds(nv + ng), acc((size_t)WG3_THREADS * 10 * MT * 4);
    float* const s_v = lds.data();
    float* const s_g = lds.data() + nv;
    for (int b = 0; b < t.grid; ++b) {
        int slab, ct, cit;
        wg3_decode_block(t, b, slab, ct, cit);
        const int co0 = ct * BM, ci0 = cit * WG3_CI;
        const bool bias = cit == 0;
        std::fill(lds.begin(), lds.end(), 0.f);
        std::fill(acc.begin(), acc.end(), 0.f);
        const int s_begin = slab * t.per;
        const int s_end = s_begin + t.per < t.S ? s_begin + t.per : t.S;
        for (int s = s_begin; s < s_end; ++s) {
            const int n = s / t.nrb;
            const int y0 = (s - n * t.nrb) * t.R;
            for (int tid = 0; tid < WG3_THREADS; ++tid) {
                for (Wg3Walk w = wg3_walk_begin(tid, t.W2, t.R + 2); w.ch < WG3_CI; wg3_walk_next(w)) {
                    if (w.row >= t.R + 2 || w.col >= t.W2) return SDA_E_LDS;
                    s_v[(size_t)w.ch * t.vp + w.row * t.W2 + w.col] = wg3_stage_v(d, t, n, y0, ci0 + w.ch, w.row, w.col);
                }
                for (Wg3Walk w = wg3_walk_begin(tid, t.W2, t.R); w.ch < BM; wg3_walk_next(w)) {
                    if (w.row >= t.R || w.col >= t.W2) return SDA_E_LDS;
                    s_g[(size_t)w.ch * t.gp + w.row * t.W2 + w.col] = wg3_stage_g(wd, t, n, y0, co0 + w.ch, w.row, w.col);
                }
            }
            for (int wave = 0; wave < 4; ++wave) {
                const int chalf = wave & 1, cot0 = (wave >> 1) * MT;
                for (int q = 0; q < t.q4; q += 4)
                    for (int tap = 0; tap < 10; ++tap) {          // tap 9: the ones column
                        if (tap == 9 && !(bias && chalf == 0)) continue;
                        for (int m = 0; m < MT; ++m) {
                            float A[16][4], B[4][16];
                            for (int lane = 0; lane < 64; ++lane) {
                                const int l15 = lane & 15, kq = lane >> 4;
                                const size_t ia = (size_t)((cot0 + m) * 16 + l15) * t.gp + kq + q;
                                if (ia >= ng) return SDA_E_LDS;
                                A[l15][kq] = s_g[ia];
                                if (tap < 9) {
                                    const size_t ib = (size_t)(chalf * 16 + l15) * t.vp + kq + q + wg3_tap_offset(t, tap);
                                    if (ib >= nv || kq + q + wg3_tap_offset(t, tap) >= t.vp) return SDA_E_LDS;
                                    B[kq][l15] = s_v[ib];
                                } else {
                                    B[kq][l15] = 1.f;
                                }
                            }
                            for (int lane = 0; lane < 64; ++lane)
                                for (int r = 0; r < 4; ++r) {
                                    const int i = wg3_mfma_row(r, lane), j = lane & 15;
                                    float& c = acc[(((size_t)(wave * 64 + lane) * 10 + tap) * MT + m) * 4 + r];
                                    for (int k = 0; k < 4; ++k) c = fmaf(A[i][k], B[k][j], c);
                                }
                        }
                    }
            }
        }
        for (int tid = 0; tid < WG3_THREADS; ++tid) {
            const int lane = tid & 63, wave = tid >> 6, l15 = lane & 15;
            const int chalf = wave & 1, cot0 = (wave >> 1) * MT;
            const int ci = ci0 + chalf * 16 + l15;
            for (int m = 0; m < MT; ++m)
                for (int r = 0; r < 4; ++r) {
                    const int co = co0 + (cot0 + m) * 16 + wg3_mfma_row(r, lane);
                    float* const o = wd.work + ((int64_t)slab * d.cout + co) * g.ncol;
                    for (int tap = 0; tap < 9; ++tap) o[ci * 9 + tap] = acc[(((size_t)tid * 10 + tap) * MT + m) * 4 + r];
                    if (bias && chalf == 0 && l15 == 0) o[g.ncol - 1] = acc[(((size_t)tid * 10 + 9) * MT + m) * 4 + r];
                }
        }
    }
    const int64_t total = (int64_t)d.cout * g.ncol;
    for (int64_t e = 0; e < total; ++e) wgrad_reduce_one(wd, g, e);
    return SDA_OK;
}
#endif  // SDA_HOST_EMU
