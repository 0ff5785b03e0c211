// The device helpers of the whole-MLP kernel texts (mlp1d_kernels.hpp: forward; mlp1d_vjp_kernels.hpp: input VJP), included by csrc/mlp1d.hip
// (both texts, rows and window mode) and csrc/mlp_train.hip (the VJP text, with its cotangent-stream hook filled in): slab staging, the multiply ml_mm, LayerNorm and its adjoint, row loaders / stores, window
// mode, the wide kernels' unit walk and the descriptor check.  See the header of mlp1d.hip for the design.
#pragma once
#include "sda_common.hpp"
#include "guide.hpp"
#include <stdlib.h>
#include <type_traits>

#define ML_SLAB (8 * 8 * 256)          // floats of the largest slab (128 x 128)
#define ML_PIECE 4096                  // floats per staging piece (1024 float4: four per thread)
#define ML_BIAS 4096                   // floats of the bias region behind the two slab buffers (every GEMM's padded bias)

typedef float ml_f32x4 __attribute__((ext_vector_type(4)));

#ifndef ML_T0                          // (the cycle stamps of a tooling build are mlp1d.hip's: it defines them in front of this header)
#define ML_T0() do {} while (0)
#define ML_STAMP(k) do {} while (0)
#define ML_DUMP() do {} while (0)
#endif

// padded sizes: an output width -> 16 or 128 features (1 or 8 D fragments); a contraction length -> 16 / 64 / 128 (1 / 4 / 8 K quads)
__host__ __device__ __forceinline__ int ml_mf(int out_f) { return out_f <= 16 ? 1 : 8; }
__host__ __device__ __forceinline__ int ml_kq(int in_f) { return in_f <= 16 ? 1 : (in_f <= 64 ? 4 : 8); }
// floats of a GEMM's slab in MEMORY: the matrix, zero padded to whole staging pieces
__host__ __device__ __forceinline__ int ml_slab_floats(int in_f, int out_f) { return (ml_mf(out_f) * ml_kq(in_f) * 256 + ML_PIECE - 1) / ML_PIECE * ML_PIECE; }

struct MlCtx {
    int tid, lane, wave, kq, li;
    int64_t row;                       // this lane's row (li of the wave's 16)
    bool rowok;
};

// copies pieces [first, first + n) x 256 float4 of the next slab global -> LDS (16-byte loads, then 16-byte stores: no vector ALU);
// issue() and commit() bracket the multiplies the copy hides behind
__device__ __forceinline__ __amdgpu_buffer_rsrc_t ml_rsrc(const float* p) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), (short)0, 0x7fffffff, 0x00020000);
}
struct MlStage {
    __amdgpu_buffer_rsrc_t src; unsigned toff;             // the slab as a buffer resource + the thread's byte offset: the piece and register
                                                           // offsets go in the scalar offset operand (a per-thread 64-bit pointer cost 8 VALU per quad)
    ml_f32x4* dst;                                         // (already offset by the thread id)
    int npieces;                                           // whole pieces of 1024 float4 (slabs are padded to that in memory)
    // A piece's four registers are LOCAL to the multiply that stages it (`sv[piece]` in ml_mm), never members that live across multiplies:
    // the loads sit under a run-time condition (this quad has a piece or not), and a register that carries an older value into that
    // condition comes out of it as a phi -- 16 v_mov_b64 per K quad on a SIMD whose vector ALU the MFMAs own.  Undefined on the other path,
    // it is just the load's destination.  (No bounds checks or per-load index arithmetic either; issuing ALL of a slab's loads up front and
    // committing four quads later measured slower: 16 loads in flight per lane.)
    __device__ __forceinline__ void issue(ml_f32x4 (&v)[4], int piece) const {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            v[i] = __builtin_bit_cast(ml_f32x4, __builtin_amdgcn_raw_buffer_load_b128(src, toff, piece * 16384 + 4096 * i, 0));
    }
    // The LDS stores are inline asm: a conditional LDS instruction the compiler can see makes it lose count of what is outstanding -- it
    // then waits lgkmcnt(0) in front of every quad's MFMAs.  Hidden from it, the count it keeps (the eight A reads) stays exact: hidden
    // stores only add to what is outstanding, so its waits are at worst early; the slab is read only behind the hand-off barrier, whose
    // s_waitcnt lgkmcnt(0) covers the stores.
    __device__ __forceinline__ void commit(const ml_f32x4 (&v)[4], int piece) const {
        const unsigned a = (unsigned)(uintptr_t)(dst + piece * 1024);      // (LDS byte address: the low 32 bits of the generic pointer)
#pragma unroll
        for (int i = 0; i < 4; ++i) asm volatile("ds_write_b128 %0, %1 offset:%2" :: "v"(a), "v"(v[i]), "n"(4096 * i) : "memory");
    }
};

template <int I, int N, class F>
__device__ __forceinline__ void ml_static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        ml_static_for<I + 1, N>(f);
    }
}

// acc[m] = sum_s A(m, s) h[s >> 2][s & 3] over the KQ K quads; A from the LDS slab `wl` ([m][sq][lane][4]).  The next slab is staged in
// pieces of 1024 float4 between the K quads (`npieces` in all; more pieces than quads: the rest follow the last one).
#ifndef SDA_ML_VAR
#define SDA_ML_VAR 0      // (tooling: 1 = no slab commits, 2 = no A reads, 4 = no slab loads -- timing only, results are wrong)
#endif
template <int MF, int KQ>
__device__ __forceinline__ void ml_mm(const float* wl, const ml_f32x4 (&h)[8], ml_f32x4 (&acc)[8], const ml_f32x4 (&cinit)[8], MlStage& st,
                                      const MlCtx& c, float* sp, const ml_f32x4 (&sreg)[8]) {
    const ml_f32x4* wa = reinterpret_cast<const ml_f32x4*>(wl) + c.lane;
    const int npieces = st.npieces;
    ml_f32x4 A[2][MF];
    ml_f32x4 sv[KQ][4];                                    // (staging registers of piece sq: live from quad sq to quad sq + 1 only)
#pragma unroll
    for (int m = 0; m < MF; ++m) A[0][m] = wa[(m * KQ) * 64];
    ml_static_for<0, KQ>([&](auto SQ_) {
        constexpr int sq = decltype(SQ_)::value;
        // The NEXT quad's A fragments are requested first (a whole quad of MFMAs, 1024 cycles, to arrive; left to itself the scheduler
        // sinks them behind the 27th MFMA and the next quad opens on their latency).  The staging -- commit the piece loaded a quad ago,
        // load this quad's -- sits in the MIDDLE of the quad's MFMAs: the LDS counter retires in order and the compiler does not see the
        // commit's stores, so its wait for these A fragments at the top of the next quad also covers the stores -- half a quad old by then.
        if (sq + 1 < KQ && !(SDA_ML_VAR & 2)) {
#pragma unroll
            for (int m = 0; m < MF; ++m) A[(sq + 1) & 1][m] = wa[(m * KQ + sq + 1) * 64];
        }
        __builtin_amdgcn_sched_barrier(0);
        auto mfmas = [&](int r) {
#pragma unroll
            for (int m = 0; m < MF; ++m) {
                // (the accumulators start from `cinit` -- the bias -- instead of zero: no add in the epilogue)
                const ml_f32x4 cin = (sq == 0 && r == 0) ? cinit[m] : acc[m];
                acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[sq & 1][m][r], h[sq][r], cin, 0, 0, 0);
            }
        };
        mfmas(0); mfmas(1);
        __builtin_amdgcn_sched_barrier(0);
#if !(SDA_ML_VAR & 1)
        if constexpr (sq >= 1) { if (sq - 1 < npieces) st.commit(sv[sq - 1], sq - 1); }
#endif
#if !(SDA_ML_VAR & 4)
        if (sq < npieces) st.issue(sv[sq], sq);
#endif
        // one 16-byte store of a saved stream (the block input or the pre-activation, for the VJP) per quad: in a burst in the epilogue
        // the 16 stores per lane queue behind the CU's 64 B/clk store path with nothing else for the wave to do (~11 000 cycles of a
        // tile's 172 000, and the waves reach the hand-off barrier apart); one per 32 MFMAs never queues
        if constexpr (MF == 8 && KQ == 8) { if (sp) *reinterpret_cast<ml_f32x4*>(sp + 16 * sq) = sreg[sq]; }
        __builtin_amdgcn_sched_barrier(0);
        mfmas(2); mfmas(3);
        __builtin_amdgcn_sched_barrier(0);
    });
    if (KQ - 1 < npieces) st.commit(sv[KQ - 1], KQ - 1);
    for (int p = KQ; p < npieces; ++p) { ml_f32x4 t[4]; st.issue(t, p); st.commit(t, p); }
#pragma unroll
    for (int m = MF; m < 8; ++m) acc[m] = ml_f32x4{0.f, 0.f, 0.f, 0.f};
}

// the one run-time (mf, kq) -> ml_mm<MF, KQ> choice (fragment / K-quad counts as ml_mf / ml_kq pad them).  The save stream `sp` is honoured
// by <8, 8> alone, the only shape that takes one: callers pass it only for 128 -> 128
__device__ __forceinline__ void ml_mm_pick(int mf, int kq, const float* wl, const ml_f32x4 (&h)[8], ml_f32x4 (&acc)[8], const ml_f32x4 (&cinit)[8],
                                           MlStage& st, const MlCtx& c, float* sp, const ml_f32x4 (&sreg)[8]) {
    if (mf == 8) {
        if (kq == 8) ml_mm<8, 8>(wl, h, acc, cinit, st, c, sp, sreg);
        else if (kq == 4) ml_mm<8, 4>(wl, h, acc, cinit, st, c, nullptr, sreg);
        else ml_mm<8, 1>(wl, h, acc, cinit, st, c, nullptr, sreg);
    } else {
        if (kq == 8) ml_mm<1, 8>(wl, h, acc, cinit, st, c, nullptr, sreg);
        else if (kq == 4) ml_mm<1, 4>(wl, h, acc, cinit, st, c, nullptr, sreg);
        else ml_mm<1, 1>(wl, h, acc, cinit, st, c, nullptr, sreg);
    }
}
__device__ __forceinline__ void ml_gemm(const float* wl, int in_f, int out_f, const ml_f32x4 (&h)[8], ml_f32x4 (&acc)[8],
                                        const ml_f32x4 (&cinit)[8], MlStage& st, const MlCtx& c, float* sp, const ml_f32x4 (&sreg)[8]) {
    ml_mm_pick(ml_mf(out_f), ml_kq(in_f), wl, h, acc, cinit, st, c, sp, sreg);
}

// a GEMM's descriptor entries.  They are read from the kernel-argument segment by a run-time index -- scalar loads, ~300 cycles each time
// the loop needs them right away; the loops keep the current and the next GEMM's in registers and fetch the one after next's while a GEMM
// multiplies (14 GEMMs per tile: ~10 000 of a tile's 168 000 cycles were this set-up)
struct MlMeta { int kind, in_f, out_f, b_off, w_off; };
__device__ __forceinline__ MlMeta ml_meta(const sda_mlp_desc& d, int g) {
    g = g < 0 ? 0 : (g >= d.ngemm ? d.ngemm - 1 : g);
    return MlMeta{d.kind[g], d.in_f[g], d.out_f[g], d.b_off[g], d.w_off[g]};
}

__device__ __forceinline__ void ml_ctx(MlCtx& c, const sda_mlp_desc& d) {
    c.tid = threadIdx.x; c.lane = c.tid & 63; c.wave = __builtin_amdgcn_readfirstlane(c.tid >> 6); c.kq = c.lane >> 4; c.li = c.lane & 15;
    c.row = (int64_t)blockIdx.x * 64 + 16 * c.wave + c.li;
    c.rowok = c.row < d.rows;
}

// sum over the features of a row: the row's values sit in the 4 lanes (kq) with this li -- two shuffles
__device__ __forceinline__ float ml_rowsum(float s) {
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    return s;
}

// LayerNorm over a row's features (4 lanes x 4 NF registers): h = (a - mean) rstd, two passes.  FULL: the width fills its fragments (128 of
// 128, 256 of 256): no per-value masks -- vector-ALU instructions are what these kernels' time outside the MFMAs is made of (2.4 per MFMA in
// the first version, rocprofv3 SQ_INSTS_VALU).  The kernels pick FULL through a generic lambda (`ln`, `lnb`, as `epi` / `dact` pick the
// activation): called bare from the narrow kernels' loops, the same helper compiled to 184-264 more instructions per forward kernel.
template <bool FULL, int NF>
__device__ __forceinline__ void ml_ln(const ml_f32x4 (&a)[NF], ml_f32x4 (&h)[NF], int cw, const MlCtx& c, float inv_c, float inv_v, float eps,
                                      float& mean, float& rstd) {
    float s = 0.f;
#pragma unroll
    for (int m = 0; m < NF; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) s += (FULL || 16 * m + 4 * c.kq + r < cw) ? a[m][r] : 0.f;
    mean = ml_rowsum(s) * inv_c;
    s = 0.f;
#pragma unroll
    for (int m = 0; m < NF; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float dl = a[m][r] - mean;
            h[m][r] = dl;
            s += (FULL || 16 * m + 4 * c.kq + r < cw) ? dl * dl : 0.f;
        }
    rstd = __builtin_amdgcn_rsqf(ml_rowsum(s) * inv_v + eps);
#pragma unroll
    for (int m = 0; m < NF; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) h[m][r] = (FULL || 16 * m + 4 * c.kq + r < cw) ? h[m][r] * rstd : 0.f;
}
// its adjoint: g += LN^T(gh) = rstd (gh - mean_c(gh) - x_hat mean'_c(gh x_hat)); sv = the block input on entry, x_hat on return
template <bool FULL, int NF>
__device__ __forceinline__ void ml_ln_bwd(ml_f32x4 (&sv)[NF], const ml_f32x4 (&acc)[NF], ml_f32x4 (&gacc)[NF], int cw, const MlCtx& c,
                                          float inv_c, float inv_v, float mean, float rs) {
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int m = 0; m < NF; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool fok = FULL || 16 * m + 4 * c.kq + r < cw;
            const float xh = fok ? (sv[m][r] - mean) * rs : 0.f;
            sv[m][r] = xh;
            const float gv = fok ? acc[m][r] : 0.f;
            s1 += gv; s2 += gv * xh;
        }
    const float av_ = ml_rowsum(s1) * inv_c, bv_ = ml_rowsum(s2) * inv_v;
#pragma unroll
    for (int m = 0; m < NF; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool fok = FULL || 16 * m + 4 * c.kq + r < cw;
            gacc[m][r] += fok ? rs * (acc[m][r] - av_ - sv[m][r] * bv_) : 0.f;
        }
}

// the wave's rows x `width` features of a row-major source -> D-layout registers h[m][r] = x[row][16 m + 4 kq + r] (zero beyond)
template <int NF>
__device__ __forceinline__ void ml_load_rows(const float* src, int64_t ld, int width, const MlCtx& c, ml_f32x4 (&h)[NF]) {
    const float* xr = src + (c.rowok ? c.row : 0) * ld;
    const int nm = width <= 16 ? 1 : (width <= 64 ? 4 : ((NF == 8 || width <= 128) ? 8 : 16));
#pragma unroll
    for (int m = 0; m < NF; ++m) {
        h[m] = ml_f32x4{0.f, 0.f, 0.f, 0.f};
        if (m < nm) {                                      // (wave uniform)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = 16 * m + 4 * c.kq + r;
                const float v = xr[f < width ? f : 0];
                h[m][r] = (c.rowok && f < width) ? v : 0.f;
            }
        }
    }
}

template <int NF>
__device__ __forceinline__ void ml_store_rows(float* dst, int64_t ld, int width, const MlCtx& c, const ml_f32x4 (&v)[NF]) {
    if (!c.rowok) return;
    float* o = dst + c.row * ld;
    const int nm = width <= 16 ? 1 : ((NF == 8 || width <= 128) ? 8 : 16);
#pragma unroll
    for (int m = 0; m < NF; ++m)
        if (m < nm) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = 16 * m + 4 * c.kq + r;
                if (f < width) o[f] = v[m][r];
            }
        }
}

// ---- window mode (MCScoreNet over a ScoreNet kernel, sda/score.py:134-164): the rows are the windows of B trajectories; the gather
// (`unfold`), the concatenation with the time embedding (score.py:57-62), `fold` and the Gaussian-likelihood glue of GaussianScore
// (score.py:387-392) are the loader and the epilogue of the launch -- see sda_mlp_fwd_win / sda_mlp_bwd_win in sda_hip.h.
struct MlWinRow { int b, i; bool first, lastw; };
__device__ __forceinline__ MlWinRow ml_win_row(const sda_mlp_win& w, const MlCtx& c) {
    MlWinRow r;
    const int64_t row = c.rowok ? c.row : 0;
    r.b = (int)(row / w.nw); r.i = (int)(row - (int64_t)r.b * w.nw);
    r.first = r.i == 0; r.lastw = r.i == w.nw - 1;
    return r;
}
// does `fold` read slot j of this window?  (the centre always; the leading slots of a trajectory's first window, the trailing ones of its last)
__device__ __forceinline__ bool ml_win_sel(const MlWinRow& r, int j, int k) { return j == k || (r.first && j < k) || (r.lastw && j > k); }

// the forward loader of window mode: the wave's rows in D layout.  (The wide kernels' only: mlp_fwd_kernel<true> keeps an inline copy of it, as
// mlp_bwd_kernel<true> does of ml_win_cot below -- called from there these two compile to 3 and 43 instructions more than the copies, and no
// timing of that exists.  An edit of one belongs in its copy.)
template <int NF>
__device__ __forceinline__ void ml_win_load(const sda_mlp_win& w, const MlCtx& c, ml_f32x4 (&a)[NF]) {
    // row (b, i): features [0, WC) = x[b][i .. i + 2k][:] -- WC consecutive floats of the trajectory --, then the time embedding
    const MlWinRow wr = ml_win_row(w, c);
    const int wc = (w.len - w.nw + 1) * w.c;
    const float* xr = w.x + ((int64_t)wr.b * w.len + wr.i) * w.c;
#pragma unroll
    for (int m = 0; m < NF; ++m) {
        if (NF > 8 && 16 * m >= wc + w.emb_n) { a[m] = ml_f32x4{0.f, 0.f, 0.f, 0.f}; continue; }   // (wave uniform; the wide kernels only)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int f = 16 * m + 4 * c.kq + r;
            const bool isx = f < wc, ise = !isx && f < wc + w.emb_n;
            const float xv = xr[isx ? f : 0], ev = w.emb[ise ? f - wc : 0];
            a[m][r] = !c.rowok ? 0.f : (isx ? xv : (ise ? ev : 0.f));
        }
    }
}
// the forward epilogue of window mode; a = the wave's output fragments, of which the first WF (1: a window of at most 16 values, 2: of 17 .. 32)
// hold the window values of a row.  (WF = 1 is the code of the one-fragment version, value for value.)
template <int WF, int NF>
__device__ __forceinline__ void ml_win_fold(const sda_mlp_win& w, const MlCtx& c, const ml_f32x4 (&a)[NF]) {
    // fold (score.py:155-164) + eps = (cx0 + cx1 sigma) x + cn s + the likelihood cotangent: guide.hpp's arithmetic, as sda_net1d_fwd_fused's epilogue
    if (c.rowok) {
        const MlWinRow wr = ml_win_row(w, c);
        const int k = (w.len - w.nw) / 2, wc = (2 * k + 1) * w.c;
        const SdaGuide g = sda_guide_of(w);
        const SdaLattice obs = sda_lattice_of(w);
        const float* yb = w.y + (int64_t)wr.b * w.y_sn;
#pragma unroll
        for (int m = 0; m < WF; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = 16 * m + 4 * c.kq + r;
                if (f >= wc) continue;
                const int j = f / w.c, ch = f - j * w.c;
                if (!ml_win_sel(wr, j, k)) continue;
                const int ps = wr.i + j;
                const int64_t o = ((int64_t)wr.b * w.len + ps) * w.c + ch;
                const float xv = w.x[o];
                const float e = g.eps_of(xv, a[m][r]);
                w.eps[o] = e;
                float gv = 0.f;
                if (obs.at(ps, ch)) {
                    const float xh = g.xhat(xv, e);
                    gv = g.cot(yb[obs.y_index(ps, ch)], xh);
                }
                w.ghat[o] = gv;
            }
    }
}
// the VJP's loader of window mode
template <int WF, int NF>
__device__ __forceinline__ void ml_win_cot(const sda_mlp_win& w, const MlCtx& c, ml_f32x4 (&gacc)[NF]) {
    // the cotangent of the window outputs = fold's adjoint of cn ghat: slot j of window (b, i) receives ghat[b][i + j] where fold reads it
    const MlWinRow wr = ml_win_row(w, c);
    const int k = (w.len - w.nw) / 2, wc = (2 * k + 1) * w.c;
#pragma unroll
    for (int m = 0; m < NF; ++m) gacc[m] = ml_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < WF; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int f = 16 * m + 4 * c.kq + r, fc = f < wc ? f : 0;
            const int j = fc / w.c, ch = fc - j * w.c;
            const bool sel = c.rowok && f < wc && ml_win_sel(wr, j, k);
            const float gv = w.ghat[sel ? ((int64_t)wr.b * w.len + wr.i + j) * w.c + ch : 0];
            gacc[m][r] = sel ? gv * w.cn : 0.f;
        }
}
// the VJP's store of window mode: the window part of the input gradient, gwin[row][16 WF] (a row's stride follows its window: 16 floats up
// to 16 values, 32 above -- sda_mc_finish reads it by the same rule)
template <int WF, int NF>
__device__ __forceinline__ void ml_win_gstore(const sda_mlp_win& w, const MlCtx& c, const ml_f32x4 (&gacc)[NF]) {
    if (!c.rowok) return;
#pragma unroll
    for (int m = 0; m < WF; ++m) *reinterpret_cast<ml_f32x4*>(w.gwin + c.row * (16 * WF) + 16 * m + 4 * c.kq) = gacc[m];
}

// ------------------------------------------------------------------------------------------------------------ wide nets (a width in 129 .. 256)
// See the file header ("Wide nets").  A GEMM is NH x KH UNITS -- ordinary slabs of at most 128 x 128 -- that follow each other in memory in the
// order [n half][k half] and through the two LDS buffers exactly as whole GEMMs do in the kernels above: unit u multiplies out of buffer u & 1
// while ml_mm copies unit u + 1 into the other one; one barrier per unit.
__host__ __device__ __forceinline__ int mlw_mf(int out_f) { return out_f <= 128 ? ml_mf(out_f) : 16; }
__host__ __device__ __forceinline__ int mlw_kq(int in_f) { return in_f <= 128 ? ml_kq(in_f) : 16; }
// floats of one unit of GEMM (in_f -> out_f) in memory (all units of a GEMM have one shape), and of the whole GEMM
__host__ __device__ __forceinline__ int mlw_unit_floats(int in_f, int out_f) { return ml_slab_floats(in_f > 128 ? 128 : in_f, out_f > 128 ? 128 : out_f); }
__host__ __device__ __forceinline__ int mlw_slab_floats(int in_f, int out_f) {
    return (in_f > 128 ? 2 : 1) * (out_f > 128 ? 2 : 1) * mlw_unit_floats(in_f, out_f);
}

// unit (NH, KH) of a GEMM: acc[8 NH ..] (+)= A h[8 KH ..]; `mfu` / `kqu` = the unit's fragment / K-quad counts (8 wherever the GEMM has a
// second half on that axis -- a compile-time 8 for NH / KH = 1: 12 inlined ml_mm bodies over the four unit positions)
template <int NH, int KH>
__device__ __forceinline__ void mlw_unit(const float* wl, int mfu, int kqu, const ml_f32x4 (&h)[16], ml_f32x4 (&acc)[16],
                                         const ml_f32x4 (&cinit)[8], MlStage& st, const MlCtx& c) {
    const ml_f32x4 (&hk)[8] = *reinterpret_cast<const ml_f32x4 (*)[8]>(&h[8 * KH]);
    ml_f32x4 (&an)[8] = *reinterpret_cast<ml_f32x4 (*)[8]>(&acc[8 * NH]);
    ml_mm_pick(NH == 1 ? 8 : mfu, KH == 1 ? 8 : kqu, wl, hk, an, cinit, st, c, nullptr, hk);
}

// one GEMM (in_f -> out_f, slab at `ws`): acc = W h.  `nsrc` / `npieces` = the first unit of the NEXT GEMM (staged under this one's last
// unit); `buf` = the LDS buffer that holds this GEMM's first unit.
__device__ __forceinline__ void mlw_gemm(float* lds, int& buf, const float* ws, int in_f, int out_f, const float* nsrc, int npieces,
                                         const ml_f32x4 (&h)[16], ml_f32x4 (&acc)[16], MlStage& st, const MlCtx& c) {
    const int nhn = out_f > 128 ? 2 : 1, khn = in_f > 128 ? 2 : 1;
    const int mfu = nhn == 2 ? 8 : ml_mf(out_f), kqu = khn == 2 ? 8 : ml_kq(in_f);
    const int usz = mlw_unit_floats(in_f, out_f);
    ml_static_for<0, 4>([&](auto U_) {
        constexpr int NH = decltype(U_)::value >> 1, KH = decltype(U_)::value & 1;
        if (NH < nhn && KH < khn) {                        // (wave uniform)
            const bool lastu = NH == nhn - 1 && KH == khn - 1;
            st.src = ml_rsrc(lastu ? nsrc : ws + (NH * khn + KH + 1) * usz);
            st.dst = reinterpret_cast<ml_f32x4*>(lds + (buf ^ 1) * ML_SLAB) + c.tid;
            st.npieces = lastu ? npieces : usz / ML_PIECE;
            const float* wl = lds + buf * ML_SLAB;
            if constexpr (KH == 0) {
                const ml_f32x4 zero[8] = {};
                mlw_unit<NH, KH>(wl, mfu, kqu, h, acc, zero, st, c);
            } else {
                // the second K half accumulates on the first one's sums
                mlw_unit<NH, KH>(wl, mfu, kqu, h, acc, *reinterpret_cast<const ml_f32x4 (*)[8]>(&acc[8 * NH]), st, c);
            }
            __syncthreads();                               // unit hand-off: the next unit is complete, this one's buffer is free
            buf ^= 1;
        }
    });
    if (nhn == 1) {
#pragma unroll
        for (int m = 8; m < 16; ++m) acc[m] = ml_f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// `wide`: a width above 128 -- the net runs the _wide kernels
static inline int mlp_check(const sda_mlp_desc* d, bool bwd, bool win, bool* wide) {
    if (!d || d->rows < 1 || d->ngemm < 1 || d->ngemm > SDA_MLP_MAXG) return SDA_E_UNSUPPORTED;
    if ((!win && (!d->x || !d->out)) || !d->w || (!bwd && !d->bias)) return SDA_E_BADARG;
    int nres = 0, wmax = 0, wres = 0;
    for (int g = 0; g < d->ngemm; ++g) {
        if (d->in_f[g] < 1 || d->out_f[g] < 1 || d->in_f[g] > 256 || d->out_f[g] > 256 || d->kind[g] < 0 || d->kind[g] > 2) return SDA_E_UNSUPPORTED;
        if (g > 0 && d->in_f[g] != d->out_f[g - 1]) return SDA_E_BADARG;
        if (d->kind[g] == 1) {
            if (g + 1 >= d->ngemm || d->kind[g + 1] != 2 || d->in_f[g] != d->out_f[g] || d->out_f[g + 1] != d->in_f[g]) return SDA_E_BADARG;
            if (d->unbiased && d->in_f[g] < 2) return SDA_E_UNSUPPORTED;
            ++nres;
            if (d->in_f[g] > wres) wres = d->in_f[g];
        }
        if (d->in_f[g] > wmax) wmax = d->in_f[g];
        if (d->out_f[g] > wmax) wmax = d->out_f[g];
        if (d->kind[g] == 2 && (g == 0 || d->kind[g - 1] != 1)) return SDA_E_BADARG;
        if ((d->w_off[g] & 3) || (d->b_off[g] & 3)) return SDA_E_BADARG;
    }
    if ((reinterpret_cast<uintptr_t>(d->w) & 15) || (!bwd && (reinterpret_cast<uintptr_t>(d->bias) & 15))) return SDA_E_BADARG;
    *wide = wmax > 128;
    // (every GEMM's padded bias sits in LDS for the whole launch: 4096 floats -- sixteen 256-wide GEMMs)
    if (!bwd && d->b_off[d->ngemm - 1] + 16 * mlw_mf(d->out_f[d->ngemm - 1]) > ML_BIAS) return SDA_E_UNSUPPORTED;
    const bool saves = d->a_save && d->z_save && d->mean_save && d->rstd_save;
    if (nres > 0) {
        if (bwd && !saves) return SDA_E_BADARG;
        if (!bwd && (d->a_save || d->z_save || d->mean_save || d->rstd_save) && !saves) return SDA_E_BADARG;
        if (saves && (d->save_ld < (wres > 128 ? 256 : 128) || (d->save_ld & 3) || (reinterpret_cast<uintptr_t>(d->a_save) & 15) ||
                      (reinterpret_cast<uintptr_t>(d->z_save) & 15) || (d->save_stride & 3)))
            return SDA_E_BADARG;
    }
    return SDA_OK;
}
