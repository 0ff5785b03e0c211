// Weight gradient of the 3 x 3 convolutions of a 2-D U-Net: the tiled route beside the general kernel (conv_wgrad.hip), one kernel
// template for three geometries (s = stride; up2 reads V through the nearest-neighbour up-sampling).
//
//   dW[co][ci][ky][kx] = sum_{n,oy,ox} g[n][co][oy][ox] * V(n, ci, oy s + ky - 1, ox s + kx - 1),   db[co] = sum g
//
// Served: 2-D, kh = kw = 3, no zero insertion / pooling, no context channels, no explicit pad, planar contiguous source,
// cx % 32 == 0, cout % 32 == 0, circular or zero padding, and one of
//   s1  (sda_conv_wgrad3_serves, the block convolutions): stride 1, no up-sampling, ho = hs, wo = ws, loader = LayerNorm +
//       modulation (conv1), activation (conv2) or none;
//   up2 (sda_conv_wgrad3x_serves, the tails): up_h = up_w = 2, stride 1, ho = 2 hs, wo = 2 ws, loader = LayerNorm without
//       modulation or activation, or none;
//   s2  (sda_conv_wgrad3x_serves, the heads): stride_h = stride_w = 2, no up-sampling, hs and ws even, ho = hs / 2, wo = ws / 2,
//       plain loader.
// Everything else, and a geometry of the other entry's set: SDA_E_UNSUPPORTED (the general kernel serves it).
//
// Design (H, W are the OUTPUT size, W2 = W + 2):
//   * a stage is R output rows of one image, all W columns.  The workgroup (4 waves) stages the input image of its 32 channels
//     ONCE, halo included (wrap / zero padding and the loader's LayerNorm / modulation / activation applied here, through the
//     general kernel's own loader helper), and the cotangent as g[BM][R x W2] with the two pad columns of every row zero: both
//     tiles then share one position index q = r W2 + ox, and the B operand of tap (ky, kx) is the V tile read at q + off(ky, kx)
//     -- nine shifted reads of one tile instead of nine staged copies.  The two staged images:
//       s1, up2: V[32][(R + 2) x W2], the rows y0 - 1 .. y0 + R and columns -1 .. W of the (s1) source, (up2) up-sampled grid:
//                element (row, col) is the loader's value at the source pixel (y >> sh, x >> sh), sh = 0 / 1, after the wrap /
//                zero test in output coordinates.  off = ky W2 + kx;
//       s2:      the input rows 2 y0 - 1 .. 2 (y0 + R) - 1 as four parity planes, plane (py, px) row t column u = input pixel
//                (2 (y0 + t) - py, 2 u - px), each R + 1 rows of pitch W2 (pp floats).  off = plane((ky + 1) & 1, (kx + 1) & 1) pp +
//                (ky == 2) W2 + (kx == 2).  hs and ws even: only row -1 and column -1 wrap or pad, never the far border;
//   * v_mfma_f32_16x16x4_f32 with M = cout, N = cin, K = positions: A = g[co = lane&15][q = 4 ks + (lane>>4)], B = V[ci = lane&15][...],
//     D row = wg3_mfma_row(r, lane), col = lane&15.  Wave w owns the 16-channel half (w & 1) of the 32 input channels and the MT
//     16-cout tiles (w >> 1) MT ..: its g fragments are loaded once per K step and reused for all nine taps, and its 9 x MT
//     accumulator tiles (108 VGPRs at the 96-cout tile) stay in registers for the whole slab;
//   * the workgroups of the first cin tile also multiply g by a column of ones: db;
//   * LDS channel pitches are = 2 (mod 32) floats: the 16 channels x 2 positions a 32-lane half reads with ds_read_b32 fall on 32
//     different banks, whatever the tap shift; reads past a row block or plane (pad columns, the K round-up) meet a zero cotangent;
//   * the position axis (stages) is cut into slabs; a workgroup writes its tile, unreduced, to work[slab][co][ci*9 + tap] -- the
//     general kernel's column order, ones column last -- and the general kernel's slab-order reduction finishes: no atomics,
//     bitwise reproducible, `accumulate` as there.
//
// Index arithmetic is in __host__ __device__ helpers; the emulator at the bottom (libsda_emu.so, tests only) replays the planner,
// the staging walk and maps (halo, wrap, zero pad, parity planes), the tap offsets, the MFMA lane maps and the reduction order on
// the CPU.
#include "conv_wgrad.hpp"

#define WG3_THREADS 256
#define WG3_CI 32                 // input channels per workgroup
#define WG3_Q 128                 // target positions (pad columns included) per stage
#define WG3_MAX_SLABS 256
#define WG3_TARGET_BLOCKS 512     // two workgroups on each of 256 CUs
#define WG3_LDS_MAX (160 * 1024)

enum { WG3_UP2 = 0, WG3_S2 = 1, WG3_S1 = 2 };                 // (sda_conv_wgrad3x_plan reports up2 = 0, s2 = 1)
#define WG3_SET_BLOCKS (1u << WG3_S1)                         // the modes sda_conv_wgrad3 ...
#define WG3_SET_HT ((1u << WG3_UP2) | (1u << WG3_S2))         // ... and sda_conv_wgrad3x serve

struct Wg3Geom {
    int H, W, W2;        // output size, row pitch W + 2 of both tiles
    int R, nrb;          // rows per stage, row blocks per image
    int S;               // stages = n * nrb
    int per, slabs;      // stages per slab
    int mt, bm;          // cout tile = 32 mt
    int n_ct, n_cit;     // cout tiles, cin tiles
    int q4;              // K extent of a stage: R * W2 rounded up to 4
    int gp, vp;          // LDS channel pitches (floats) of the g and V tiles
    int lds_bytes;
    int grid;
    int mode;            // WG3_UP2 | WG3_S2 | WG3_S1
    int vrows;           // rows of pitch W2 staged per input channel: R + 2, s2: 4 (R + 1)
    int pp;              // s2: floats of one parity plane, (R + 1) W2
    int hs, ws;          // source size
};

__host__ __device__ inline int wg3_pitch(int need) {          // smallest pitch >= need that is 2 (mod 32)
    return (need + 29) / 32 * 32 + 2;
}

// -> SDA_OK and the plan, SDA_E_UNSUPPORTED outside the served modes of `allowed`, SDA_E_BADARG as the general planner
static int wg3_plan(const sda_wgrad_desc* wd, unsigned allowed, Wg3Geom* t, WgradGeom* g) {
    if (!wd) return SDA_E_BADARG;
    sda_wgrad_desc chk = *wd;
    chk.slabs = 0;                                            // (this route has its own slab range)
    int rc = wgrad_plan(&chk, g);
    if (rc != SDA_OK) return rc;
    const sda_conv_desc& d = wd->conv;
    if (wd->slabs < 0 || wd->slabs > WG3_MAX_SLABS) return SDA_E_BADARG;
    if (d.kh != 3 || d.kw != 3) return SDA_E_UNSUPPORTED;
    if (d.cctx > 0 || d.explicit_pad) return SDA_E_UNSUPPORTED;
    if (d.x_sx != 1 || d.x_sy != d.ws || d.x_sc != (int64_t)d.hs * d.ws || d.n_inner != 1) return SDA_E_UNSUPPORTED;
    if (d.cx % WG3_CI || d.cout % 32) return SDA_E_UNSUPPORTED;
    const bool ln = d.ln_mean != nullptr, mod = d.mod != nullptr, act = d.act_in != 0;
    const bool up1 = d.up_h == 1 && d.up_w == 1, s1 = d.stride_h == 1 && d.stride_w == 1;
    if (up1 && s1) {
        if (d.ho != d.hs || d.wo != d.ws) return SDA_E_UNSUPPORTED;
        if (!((ln && mod && !act) || (!ln && !mod))) return SDA_E_UNSUPPORTED;     // conv1 | conv2 or plain
        t->mode = WG3_S1;
    } else if (d.up_h == 2 && d.up_w == 2 && s1) {
        if (d.ho != 2 * d.hs || d.wo != 2 * d.ws) return SDA_E_UNSUPPORTED;
        if (mod || act) return SDA_E_UNSUPPORTED;             // LayerNorm alone (the tails) or plain
        t->mode = WG3_UP2;
    } else if (up1 && d.stride_h == 2 && d.stride_w == 2) {
        if ((d.hs & 1) || (d.ws & 1) || d.ho != d.hs / 2 || d.wo != d.ws / 2) return SDA_E_UNSUPPORTED;
        if (ln || mod || act) return SDA_E_UNSUPPORTED;       // plain (the heads)
        t->mode = WG3_S2;
    } else {
        return SDA_E_UNSUPPORTED;
    }
    if (!(allowed >> t->mode & 1)) return SDA_E_UNSUPPORTED;
    t->hs = d.hs;
    t->ws = d.ws;
    t->H = d.ho;                                              // (s1: the source size as well)
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
    if (t->mode == WG3_S2) {
        t->vrows = 4 * (R + 1);
        t->pp = (R + 1) * t->W2;
        t->vp = wg3_pitch(3 * t->pp + t->q4 + t->W2 + 1);     // (the last K step of tap (2, 2) reads plane 3 up to 3 pp + q4 - 1 + W2 + 1)
    } else {
        t->vrows = R + 2;
        t->pp = 0;
        t->vp = wg3_pitch(t->q4 + 2 * t->W2 + 2);             // (... reads up to q4 - 1 + 2 W2 + 2)
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

// D-fragment row of accumulator register r for v_mfma_f32_16x16x4_f32 (col = lane & 15)
__host__ __device__ inline int wg3_mfma_row(int r, int lane) { return 4 * (lane >> 4) + r; }

// workgroup b -> (slab, cout tile, cin tile)
__host__ __device__ inline void wg3_decode_block(const Wg3Geom& t, int b, int& slab, int& ct, int& cit) {
    cit = b % t.n_cit;
    int r = b / t.n_cit;
    ct = r % t.n_ct;
    slab = r / t.n_ct;
}

// The staging walk: thread tid visits the elements tid, tid + 256, ... of a [channel][row][col] tile in that order; the
// decomposition of the step is formed once, the walk itself is adds and compares.
struct Wg3Walk {
    int cols, rows;
    int dcol, drow, dch;
    int col, row, ch;
};
__host__ __device__ inline Wg3Walk wg3_walk_begin(int tid, int cols, int rows) {
    Wg3Walk w;
    w.cols = cols; w.rows = rows;
    const int units = WG3_THREADS / cols;
    w.dcol = WG3_THREADS - units * cols;
    w.dch = units / rows;
    w.drow = units - w.dch * rows;
    w.col = tid % cols;
    const int u = tid / cols;
    w.ch = u / rows;
    w.row = u - w.ch * rows;
    return w;
}
__host__ __device__ inline void wg3_walk_next(Wg3Walk& w) {
    w.col += w.dcol;
    if (w.col >= w.cols) { w.col -= w.cols; ++w.row; }
    w.row += w.drow;
    if (w.row >= w.rows) { w.row -= w.rows; ++w.ch; }
    w.ch += w.dch;
}

// element (row, col) of channel co of the staged cotangent tile: zero in the two pad columns and below the image
__host__ __device__ inline float wg3_stage_g(const sda_wgrad_desc& wd, const Wg3Geom& t, int n, int y0, int co, int row, int col) {
    const int y = y0 + row;
    if (col >= t.W || y >= t.H) return 0.f;
    return wd.g[(((int64_t)n * wd.conv.cout + co) * t.H + y) * t.W + col];
}

// s1 (SH = 0), up2 (SH = 1): element (row, col) of channel ci of the staged image of stage (n, y0): V at the output-grid pixel
// (y0 - 1 + row, col - 1), wrapped or zero-padded on that grid, read at the source pixel (y >> SH, x >> SH)
template <int SH>
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
    return wgrad_load_src(d, n, ci, y >> SH, x >> SH);
}

// s2: element (row, col) of the staged image: row = plane (R + 1) + tr, plane = 2 py + px -> the input pixel (2 (y0 + tr) - py,
// 2 col - px).  Row -1 / column -1 wrap or are padding; pixels at or past hs / ws belong to no tap of a live output position
// (2 oy + 1 <= hs - 1): zero.
__host__ __device__ inline float wg3x_stage_s2(const sda_conv_desc& d, const Wg3Geom& t, int n, int y0, int ci, int row, int col) {
    const int r1 = t.R + 1;
    const int plane = (row >= r1) + (row >= 2 * r1) + (row >= 3 * r1);        // row / r1 for row < 4 r1
    const int tr = row - plane * r1;
    int y = 2 * (y0 + tr) - (plane >> 1), x = 2 * col - (plane & 1);
    if (y >= t.hs || x >= t.ws) return 0.f;
    if (y < 0) {
        if (!d.circular) return 0.f;
        y += t.hs;
    }
    if (x < 0) {
        if (!d.circular) return 0.f;
        x += t.ws;
    }
    return wgrad_load_src(d, n, ci, y, x);
}

// the staged V element of geometry MODE
template <int MODE>
__host__ __device__ inline float wg3_stage(const sda_conv_desc& d, const Wg3Geom& t, int n, int y0, int ci, int row, int col) {
    if (MODE == WG3_S2) return wg3x_stage_s2(d, t, n, y0, ci, row, col);
    return wg3_stage_v<MODE == WG3_UP2>(d, t, n, y0, ci, row, col);
}

// LDS offset of tap (ky, kx) relative to the position index
__host__ __device__ inline int wg3_tap_offset(const Wg3Geom& t, int tap) {
    const int ky = tap / 3, kx = tap - 3 * ky;
    if (t.mode != WG3_S2) return ky * t.W2 + kx;
    const int plane = 2 * ((ky + 1) & 1) + ((kx + 1) & 1);
    return plane * t.pp + (ky == 2 ? t.W2 : 0) + (kx == 2 ? 1 : 0);
}

// ---------------------------------------------------------------- the kernel
#ifndef SDA_HOST_EMU

typedef float wg3_f32x4 __attribute__((ext_vector_type(4)));

template <int MT, int MODE>
__global__ __launch_bounds__(WG3_THREADS, 2) void conv_wgrad3_kernel(const sda_wgrad_desc wd, const Wg3Geom plan, const int ncol) {
    constexpr int BM = 32 * MT;
    Wg3Geom t = plan;
    t.mode = MODE;                                            // the instantiation's geometry, spelled out for wg3_tap_offset
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
    const Wg3Walk wv0 = wg3_walk_begin(tid, t.W2, t.vrows);
    const Wg3Walk wg0 = wg3_walk_begin(tid, t.W2, t.R);

    const int s_begin = slab * t.per;
    const int s_end = s_begin + t.per < t.S ? s_begin + t.per : t.S;
    for (int s = s_begin; s < s_end; ++s) {
        const int n = s / t.nrb;
        const int y0 = (s - n * t.nrb) * t.R;
        __syncthreads();                                      // the previous stage's reads (and the clear) are done
        for (Wg3Walk w = wv0; w.ch < WG3_CI; wg3_walk_next(w))
            s_v[w.ch * t.vp + w.row * t.W2 + w.col] = wg3_stage<MODE>(d, t, n, y0, ci0 + w.ch, w.row, w.col);
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
static int wg3_launch_t(const sda_wgrad_desc* d, const Wg3Geom& t, const WgradGeom& g, hipStream_t stream) {
    static bool raised[SDA_MAX_DEVICES];
    int rc = sda_raise_dyn_lds((const void*)conv_wgrad3_kernel<MT, MODE>, WG3_LDS_MAX, raised);
    if (rc != SDA_OK) return rc;
    hipLaunchKernelGGL((conv_wgrad3_kernel<MT, MODE>), dim3(t.grid), dim3(WG3_THREADS), t.lds_bytes, stream, *d, t, g.ncol);
    return sda_launch_status();
}

static int wg3_launch(const sda_wgrad_desc* d, unsigned allowed, void* stream) {
    Wg3Geom t;
    WgradGeom g;
    int rc = wg3_plan(d, allowed, &t, &g);
    if (rc != SDA_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    switch (3 * t.mode + t.mt) {
        case 3 * WG3_S1 + 1: rc = wg3_launch_t<1, WG3_S1>(d, t, g, st); break;
        case 3 * WG3_S1 + 2: rc = wg3_launch_t<2, WG3_S1>(d, t, g, st); break;
        case 3 * WG3_S1 + 3: rc = wg3_launch_t<3, WG3_S1>(d, t, g, st); break;
        case 3 * WG3_UP2 + 1: rc = wg3_launch_t<1, WG3_UP2>(d, t, g, st); break;
        case 3 * WG3_UP2 + 2: rc = wg3_launch_t<2, WG3_UP2>(d, t, g, st); break;
        case 3 * WG3_UP2 + 3: rc = wg3_launch_t<3, WG3_UP2>(d, t, g, st); break;
        case 3 * WG3_S2 + 1: rc = wg3_launch_t<1, WG3_S2>(d, t, g, st); break;
        case 3 * WG3_S2 + 2: rc = wg3_launch_t<2, WG3_S2>(d, t, g, st); break;
        default: rc = wg3_launch_t<3, WG3_S2>(d, t, g, st); break;
    }
    if (rc != SDA_OK) return rc;
    return wgrad_launch_reduce(d, g, st);
}

extern "C" int sda_conv_wgrad3(const sda_wgrad_desc* d, void* stream) { return wg3_launch(d, WG3_SET_BLOCKS, stream); }
extern "C" int sda_conv_wgrad3x(const sda_wgrad_desc* d, void* stream) { return wg3_launch(d, WG3_SET_HT, stream); }

#endif  // !SDA_HOST_EMU

// planning entries (host only: nothing is launched)
static int wg3_serves(const sda_wgrad_desc* d, unsigned allowed) {
    Wg3Geom t;
    WgradGeom g;
    return wg3_plan(d, allowed, &t, &g) == SDA_OK ? 1 : 0;
}

static int64_t wg3_work_floats(const sda_wgrad_desc* d, unsigned allowed) {
    Wg3Geom t;
    WgradGeom g;
    int rc = wg3_plan(d, allowed, &t, &g);
    return rc != SDA_OK ? (int64_t)rc : (int64_t)t.slabs * d->conv.cout * g.ncol;
}

extern "C" int sda_conv_wgrad3_serves(const sda_wgrad_desc* d) { return wg3_serves(d, WG3_SET_BLOCKS); }
extern "C" int sda_conv_wgrad3x_serves(const sda_wgrad_desc* d) { return wg3_serves(d, WG3_SET_HT); }
extern "C" int64_t sda_conv_wgrad3_work_floats(const sda_wgrad_desc* d) { return wg3_work_floats(d, WG3_SET_BLOCKS); }
extern "C" int64_t sda_conv_wgrad3x_work_floats(const sda_wgrad_desc* d) { return wg3_work_floats(d, WG3_SET_HT); }

// ---------------------------------------------------------------- CPU emulator (tests only; libsda_emu.so)
#ifdef SDA_HOST_EMU
#include <vector>
static int wg3_slabs(const sda_wgrad_desc* d, unsigned allowed) {
    Wg3Geom t;
    WgradGeom g;
    int rc = wg3_plan(d, allowed, &t, &g);
    return rc != SDA_OK ? rc : t.slabs;
}

// the plan as the planner made it, for the tests: {mode, R, nrb, S, mt, n_ct, n_cit, q4, vp, gp, lds_bytes, per, slabs, grid}
extern "C" int sda_conv_wgrad3x_plan(const sda_wgrad_desc* d, int* out) {
    Wg3Geom t;
    WgradGeom g;
    int rc = wg3_plan(d, WG3_SET_HT, &t, &g);
    if (rc != SDA_OK) return rc;
    const int v[14] = {t.mode, t.R, t.nrb, t.S, t.mt, t.n_ct, t.n_cit, t.q4, t.vp, t.gp, t.lds_bytes, t.per, t.slabs, t.grid};
    for (int i = 0; i < 14; ++i) out[i] = v[i];
    return SDA_OK;
}

// Replays conv_wgrad3_kernel<MT, MODE> + the shared slab reduction on the host with HOST pointers (d->work included): same
// planner, same staging walk and element maps, same tap offsets, same MFMA lane maps (A[i = l&15][k = l>>4], B[k = l>>4][j = l&15],
// D row = wg3_mfma_row(r, l), col = l&15) in the same K order.  Writes or reads outside the LDS image abort the replay with SDA_E_LDS.
static int wg3_emulate(const sda_wgrad_desc* dp, unsigned allowed) {
    Wg3Geom t;
    WgradGeom g;
    int rc = wg3_plan(dp, allowed, &t, &g);
    if (rc != SDA_OK) return rc;
    const sda_wgrad_desc& wd = *dp;
    const sda_conv_desc& d = wd.conv;
    const int MT = t.mt, BM = t.bm;
    const size_t nv = (size_t)WG3_CI * t.vp, ng = (size_t)BM * t.gp;
    if ((int)(4 * (nv + ng)) != t.lds_bytes) return SDA_E_LDS;
    if (t.vrows * t.W2 > t.vp || t.R * t.W2 > t.gp) return SDA_E_LDS;
    const auto stage = t.mode == WG3_S2 ? wg3_stage<WG3_S2> : t.mode == WG3_UP2 ? wg3_stage<WG3_UP2> : wg3_stage<WG3_S1>;
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
                for (Wg3Walk w = wg3_walk_begin(tid, t.W2, t.vrows); w.ch < WG3_CI; wg3_walk_next(w)) {
                    if (w.row >= t.vrows || w.col >= t.W2) return SDA_E_LDS;
                    s_v[(size_t)w.ch * t.vp + w.row * t.W2 + w.col] = stage(d, t, n, y0, ci0 + w.ch, w.row, w.col);
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
                                    const int iv = kq + q + wg3_tap_offset(t, tap);
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

extern "C" int sda_conv_wgrad3_slabs(const sda_wgrad_desc* d) { return wg3_slabs(d, WG3_SET_BLOCKS); }
extern "C" int sda_conv_wgrad3x_slabs(const sda_wgrad_desc* d) { return wg3_slabs(d, WG3_SET_HT); }
extern "C" int sda_conv_wgrad3_emulate(const sda_wgrad_desc* d) { return wg3_emulate(d, WG3_SET_BLOCKS); }
extern "C" int sda_conv_wgrad3x_emulate(const sda_wgrad_desc* d) { return wg3_emulate(d, WG3_SET_HT); }
#endif  // SDA_HOST_EMU
