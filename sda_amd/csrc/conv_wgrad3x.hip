// Weight gradient of the 3 x 3 stride-2 heads and up-sampling tails: the tiled route of conv_wgrad3.hip for two more geometries.
//
//   dW[co][ci][ky][kx] = sum_{n,oy,ox} g[n][co][oy][ox] * V(n, ci, oy s + ky - 1, ox s + kx - 1),   db[co] = sum g
//
// Served (sda_conv_wgrad3x_serves): 2-D, kh = kw = 3, no zero insertion / pooling, no context channels, no explicit pad, planar
// contiguous source, cx % 32 == 0, cout % 32 == 0, circular or zero padding, and one of
//   up2: up_h = up_w = 2, stride 1, ho = 2 hs, wo = 2 ws, loader = LayerNorm without modulation or activation (the tails) or none;
//   s2:  stride_h = stride_w = 2, no up-sampling, hs and ws even, ho = hs / 2, wo = ws / 2, plain loader (the heads).
// Everything else: SDA_E_UNSUPPORTED (conv_wgrad3.hip or the general kernel serves it).
//
// The plan, the cotangent tile g[BM][R x (wo + 2)], the MFMA loop (v_mfma_f32_16x16x4_f32, M = cout, N = 32 input channels, K =
// positions, 9 x MT accumulator tiles in registers for the whole slab), the ones column for db, the work layout and the slab-order
// reduction are those of conv_wgrad3.hip (H, W of the shared plan record are the OUTPUT size here).  Only the staged input image
// and the nine tap offsets into it differ; both geometries keep the one position index q = r (wo + 2) + ox:
//   up2: the image is the up-sampled tile itself, rows y0 - 1 .. y0 + R and columns -1 .. wo of the fine grid: element (row, col) is
//        the loader's value at the source pixel (y >> 1, x >> 1) after the wrap / zero test in fine coordinates.  Tap (ky, kx) reads
//        at q + ky (wo + 2) + kx, as in conv_wgrad3.hip.
//   s2:  the input rows 2 y0 - 1 .. 2 (y0 + R) - 1 as four parity planes, plane (py, px) row t column u = input pixel
//        (2 (y0 + t) - py, 2 u - px), each R + 1 rows of pitch wo + 2.  Tap (ky, kx) reads plane ((ky + 1) & 1, (kx + 1) & 1) at
//        q + (ky == 2) (wo + 2) + (kx == 2).  hs and ws even: only row -1 and column -1 wrap or pad, never the far border.
// LDS channel pitches are = 2 (mod 32) floats as there; reads past a plane (pad columns, the K round-up) meet a zero cotangent.
//
// Index arithmetic is in __host__ __device__ helpers; the emulator at the bottom (libsda_emu.so, tests only) replays the planner,
// the staging walk and maps, the tap offsets, the MFMA lane maps and the reduction order on the CPU.
#include "conv_wgrad3.hpp"

#define WG3X_UP2 0
#define WG3X_S2 1

struct Wg3xGeom {
    Wg3Geom t;           // the shared plan: H, W = output size (ho, wo)
    int mode;            // WG3X_UP2 | WG3X_S2
    int vrows;           // rows of pitch W2 staged per input channel: R + 2 (up2), 4 (R + 1) (s2)
    int pp;              // s2: floats of one parity plane, (R + 1) W2
    int hs, ws;          // source size
};

// -> SDA_OK and the plan, SDA_E_UNSUPPORTED outside the served set, SDA_E_BADARG as the general planner
static int wg3x_plan(const sda_wgrad_desc* wd, Wg3xGeom* x, WgradGeom* g) {
    if (!wd) return SDA_E_BADARG;
    sda_wgrad_desc chk = *wd;
    chk.slabs = 0;                                            // (this route has its own slab range)
    int rc = wgrad_plan(&chk, g);
    if (rc != SDA_OK) return rc;
    const sda_conv_desc& d = wd->conv;
    Wg3Geom* const t = &x->t;
    if (wd->slabs < 0 || wd->slabs > WG3_MAX_SLABS) return SDA_E_BADARG;
    if (d.kh != 3 || d.kw != 3) return SDA_E_UNSUPPORTED;
    if (d.cctx > 0 || d.explicit_pad) return SDA_E_UNSUPPORTED;
    if (d.x_sx != 1 || d.x_sy != d.ws || d.x_sc != (int64_t)d.hs * d.ws || d.n_inner != 1) return SDA_E_UNSUPPORTED;
    if (d.cx % WG3_CI || d.cout % 32) return SDA_E_UNSUPPORTED;
    const bool ln = d.ln_mean != nullptr, mod = d.mod != nullptr, act = d.act_in != 0;
    if (d.up_h == 2 && d.up_w == 2 && d.stride_h == 1 && d.stride_w == 1) {
        if (d.ho != 2 * d.hs || d.wo != 2 * d.ws) return SDA_E_UNSUPPORTED;
        if (mod || act) return SDA_E_UNSUPPORTED;             // LayerNorm alone (the tails) or plain
        x->mode = WG3X_UP2;
    } else if (d.up_h == 1 && d.up_w == 1 && d.stride_h == 2 && d.stride_w == 2) {
        if ((d.hs & 1) || (d.ws & 1) || d.ho != d.hs / 2 || d.wo != d.ws / 2) return SDA_E_UNSUPPORTED;
        if (ln || mod || act) return SDA_E_UNSUPPORTED;       // plain (the heads)
        x->mode = WG3X_S2;
    } else {
        return SDA_E_UNSUPPORTED;
    }
    x->hs = d.hs;
    x->ws = d.ws;
    t->H = d.ho;
    t->W = d.wo;
    t->W2 = d.wo + 2;
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
    if (x->mode == WG3X_UP2) {
        x->vrows = R + 2;
        x->pp = 0;
        t->vp = wg3_pitch(t->q4 + 2 * t->W2 + 2);             // (the last K step of tap (2, 2) reads up to q4 - 1 + 2 W2 + 2)
    } else {
        x->vrows = 4 * (R + 1);
        x->pp = (R + 1) * t->W2;
        t->vp = wg3_pitch(3 * x->pp + t->q4 + t->W2 + 1);     // (... of plane 3 up to 3 pp + q4 - 1 + W2 + 1; 4 pp is no more)
    }
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

// ---------------------------------------------------------------- index helpers (host + device)

// up2: element (row, col) of channel ci of the staged image of stage (n, y0): V at the fine pixel (y0 - 1 + row, col - 1), wrapped
// or zero-padded on the fine grid, read at the source pixel (y >> 1, x >> 1)
__host__ __device__ inline float wg3x_stage_up2(const sda_conv_desc& d, const Wg3xGeom& x, int n, int y0, int ci, int row, int col) {
    int y = y0 - 1 + row, xx = col - 1;                       // y in [-1, H + R), xx in [-1, W]
    if (d.circular) {
        if (y < 0) y += x.t.H;
        if (y >= x.t.H) y -= x.t.H;                           // (R <= H: once is enough)
        if (xx < 0) xx += x.t.W;
        if (xx >= x.t.W) xx -= x.t.W;
    } else if (y < 0 || y >= x.t.H || xx < 0 || xx >= x.t.W) {
        return 0.f;
    }
    return wgrad_load_src(d, n, ci, y >> 1, xx >> 1);
}

// s2: element (row, col) of the staged image: row = plane (R + 1) + t, plane = 2 py + px -> the input pixel (2 (y0 + t) - py,
// 2 col - px).  Row -1 / column -1 wrap or are padding; pixels at or past hs / ws belong to no tap of a live output position
// (2 oy + 1 <= hs - 1): zero.
__host__ __device__ inline float wg3x_stage_s2(const sda_conv_desc& d, const Wg3xGeom& x, int n, int y0, int ci, int row, int col) {
    const int r1 = x.t.R + 1;
    const int plane = (row >= r1) + (row >= 2 * r1) + (row >= 3 * r1);        // row / r1 for row < 4 r1
    const int tr = row - plane * r1;
    int y = 2 * (y0 + tr) - (plane >> 1), xx = 2 * col - (plane & 1);
    if (y >= x.hs || xx >= x.ws) return 0.f;
    if (y < 0) {
        if (!d.circular) return 0.f;
        y += x.hs;
    }
    if (xx < 0) {
        if (!d.circular) return 0.f;
        xx += x.ws;
    }
    return wgrad_load_src(d, n, ci, y, xx);
}

// LDS offset of tap (ky, kx) relative to the position index
__host__ __device__ inline int wg3x_tap_offset(const Wg3xGeom& x, int tap) {
    const int ky = tap / 3, kx = tap - 3 * ky;
    if (x.mode == WG3X_UP2) return ky * x.t.W2 + kx;
    const int plane = 2 * ((ky + 1) & 1) + ((kx + 1) & 1);
    return plane * x.pp + (ky == 2 ? x.t.W2 : 0) + (kx == 2 ? 1 : 0);
}

// ---------------------------------------------------------------- the kernel
#ifndef SDA_HOST_EMU

typedef float wg3x_f32x4 __attribute__((ext_vector_type(4)));

template <int MT, int MODE>
__global__ __launch_bounds__(WG3_THREADS, 2) void conv_wgrad3x_kernel(const sda_wgrad_desc wd, const Wg3xGeom x, const int ncol) {
    constexpr int BM = 32 * MT;
    extern __shared__ __attribute__((aligned(16))) float wg3x_lds[];
    const Wg3Geom& t = x.t;
    float* const s_v = wg3x_lds;                              // [32][vp]
    float* const s_g = wg3x_lds + WG3_CI * t.vp;              // [BM][gp]
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
    for (int i = tid; i < WG3_CI * t.vp + BM * t.gp; i += WG3_THREADS) wg3x_lds[i] = 0.f;

    wg3x_f32x4 acc[9][MT];
    wg3x_f32x4 accb[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) acc[tap][m] = (wg3x_f32x4){0.f, 0.f, 0.f, 0.f};
        accb[m] = (wg3x_f32x4){0.f, 0.f, 0.f, 0.f};
    }
    int off[9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) off[tap] = wg3x_tap_offset(x, tap);

    const float* const vb = s_v + (chalf * 16 + l15) * t.vp + kq;
    const float* const gb = s_g + (cot0 * 16 + l15) * t.gp + kq;
    const Wg3Walk wv0 = wg3_walk_begin(tid, t.W2, x.vrows);
    const Wg3Walk wg0 = wg3_walk_begin(tid, t.W2, t.R);

    const int s_begin = slab * t.per;
    const int s_end = s_begin + t.per < t.S ? s_begin + t.per : t.S;
    for (int s = s_begin; s < s_end; ++s) {
        const int n = s / t.nrb;
        const int y0 = (s - n * t.nrb) * t.R;
        __syncthreads();                                      // the previous stage's reads (and the clear) are done
        for (Wg3Walk w = wv0; w.ch < WG3_CI; wg3_walk_next(w))
            s_v[w.ch * t.vp + w.row * t.W2 + w.col] = MODE == WG3X_UP2 ? wg3x_stage_up2(d, x, n, y0, ci0 + w.ch, w.row, w.col)
                                                                       : wg3x_stage_s2(d, x, n, y0, ci0 + w.ch, w.row, w.col);
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

template <int MT, int MODE>
static int wg3x_launch_t(const sda_wgrad_desc* d, const Wg3xGeom& x, const WgradGeom& g, hipStream_t stream) {
    static bool raised[SDA_MAX_DEVICES];
    int rc = sda_raise_dyn_lds((const void*)conv_wgrad3x_kernel<MT, MODE>, WG3_LDS_MAX, raised);
    if (rc != SDA_OK) return rc;
    hipLaunchKernelGGL((conv_wgrad3x_kernel<MT, MODE>), dim3(x.t.grid), dim3(WG3_THREADS), x.t.lds_bytes, stream, *d, x, g.ncol);
    return sda_launch_status();
}

template <int MODE>
static int wg3x_launch_m(const sda_wgrad_desc* d, const Wg3xGeom& x, const WgradGeom& g, hipStream_t stream) {
    switch (x.t.mt) {
        case 1: return wg3x_launch_t<1, MODE>(d, x, g, stream);
        case 2: return wg3x_launch_t<2, MODE>(d, x, g, stream);
        default: return wg3x_launch_t<3, MODE>(d, x, g, stream);
    }
}

extern "C" int sda_conv_wgrad3x(const sda_wgrad_desc* d, void* stream) {
    Wg3xGeom x;
    WgradGeom g;
    int rc = wg3x_plan(d, &x, &g);
    if (rc != SDA_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = x.mode == WG3X_UP2 ? wg3x_launch_m<WG3X_UP2>(d, x, g, st) : wg3x_launch_m<WG3X_S2>(d, x, g, st);
    if (rc != SDA_OK) return rc;
    return wgrad_launch_reduce(d, g, st);
}

#endif  // !SDA_HOST_EMU

// planning entries (host only: nothing is launched)
extern "C" int sda_conv_wgrad3x_serves(const sda_wgrad_desc* d) {
    Wg3xGeom x;
    WgradGeom g;
    return wg3x_plan(d, &x, &g) == SDA_OK ? 1 : 0;
}

extern "C" int64_t sda_conv_wgrad3x_work_floats(const sda_wgrad_desc* d) {
    Wg3xGeom x;
    WgradGeom g;
    int rc = wg3x_plan(d, &x, &g);
    return rc != SDA_OK ? (int64_t)rc : (int64_t)x.t.slabs * d->conv.cout * g.ncol;
}

// ---------------------------------------------------------------- CPU emulator (tests only; libsda_emu.so)
#ifdef SDA_HOST_EMU
#include <vector>
extern "C" int sda_conv_wgrad3x_slabs(const sda_wgrad_desc* d) {
    Wg3xGeom x;
    WgradGeom g;
    int rc = wg3x_plan(d, &x, &g);
    return rc != SDA_OK ? rc : x.t.slabs;
}

// the plan as the planner made it, for the tests: {mode, R, nrb, S, mt, n_ct, n_cit, q4, vp, gp, lds_bytes, per, slabs, grid}
extern "C" int sda_conv_wgrad3x_plan(const sda_wgrad_desc* d, int* out) {
    Wg3xGeom x;
    WgradGeom g;
    int rc = wg3x_plan(d, &x, &g);
    if (rc != SDA_OK) return rc;
    const Wg3Geom& t = x.t;
    const int v[14] = {x.mode, t.R, t.nrb, t.S, t.mt, t.n_ct, t.n_cit, t.q4, t.vp, t.gp, t.lds_bytes, t.per, t.slabs, t.grid};
    for (int i = 0; i < 14; ++i) out[i] = v[i];
    return SDA_OK;
}

// Replays conv_wgrad3x_kernel<MT, MODE> + the shared slab reduction on the host with HOST pointers (d->work included): same
// planner, same staging walk and element maps, same tap offsets, same MFMA lane maps (A[i = l&15][k = l>>4], B[k = l>>4][j = l&15],
// D row = wg3_mfma_row(r, l), col = l&15) in the same K order.  Writes or reads outside the LDS image abort the replay with SDA_E_LDS.
extern "C" int sda_conv_wgrad3x_emulate(const sda_wgrad_desc* dp) {
    Wg3xGeom x;
    WgradGeom g;
    int rc = wg3x_plan(dp, &x, &g);
    if (rc != SDA_OK) return rc;
    const Wg3Geom& t = x.t;
    const sda_wgrad_desc& wd = *dp;
    const sda_conv_desc& d = wd.conv;
    const int MT = t.mt, BM = t.bm;
    const size_t nv = (size_t)WG3_CI * t.vp, ng = (size_t)BM * t.gp;
    if ((int)(4 * (nv + ng)) != t.lds_bytes) return SDA_E_LDS;
    if (x.vrows * t.W2 > t.vp || t.R * t.W2 > t.gp) return SDA_E_LDS;
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
                for (Wg3Walk w = wg3_walk_begin(tid, t.W2, x.vrows); w.ch < WG3_CI; wg3_walk_next(w)) {
                    if (w.row >= x.vrows || w.col >= t.W2) return SDA_E_LDS;
                    s_v[(size_t)w.ch * t.vp + w.row * t.W2 + w.col] = x.mode == WG3X_UP2
                        ? wg3x_stage_up2(d, x, n, y0, ci0 + w.ch, w.row, w.col) : wg3x_stage_s2(d, x, n, y0, ci0 + w.ch, w.row, w.col);
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
                                if (ia >= ng || kq + q >= t.gp) return SDA_E_LDS;
                                A[l15][kq] = s_g[ia];
                                if (tap < 9) {
                                    const int iv = kq + q + wg3x_tap_offset(x, tap);
                                    const size_t ib = (size_t)(chalf * 16 + l15) * t.vp + iv;
                                    if (ib >= nv || iv < 0 || iv >= t.vp) return SDA_E_LDS;
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
