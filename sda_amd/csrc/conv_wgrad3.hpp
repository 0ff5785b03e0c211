// Plan record and index helpers of the tiled 3 x 3 weight-gradient kernels, shared by conv_wgrad3.hip (stride-1 block convolutions),
// conv_wgrad3x.hip (stride-2 heads, up-sampling tails) and their host replays (libsda_emu.so).
#pragma once
#include "conv_wgrad.hpp"

#define WG3_THREADS 256
#define WG3_CI 32                 // input channels per workgroup
#define WG3_Q 128                 // target positions (pad columns included) per stage
#define WG3_MAX_SLABS 256
#define WG3_TARGET_BLOCKS 512     // two workgroups on each of 256 CUs
#define WG3_LDS_MAX (160 * 1024)

struct Wg3Geom {
    int H, W, W2;        // image size, row pitch W + 2 of both tiles
    int R, nrb;          // rows per stage, row blocks per image
    int S;               // stages = n * nrb
    int per, slabs;      // stages per slab
    int mt, bm;          // cout tile = 32 mt
    int n_ct, n_cit;     // cout tiles, cin tiles
    int q4;              // K extent of a stage: R * W2 rounded up to 4
    int gp, vp;          // LDS channel pitches (floats) of the g and V tiles
    int lds_bytes;
    int grid;
};

__host__ __device__ inline int wg3_pitch(int need) {          // smallest pitch >= need that is 2 (mod 32)
    return (need + 29) / 32 * 32 + 2;
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
