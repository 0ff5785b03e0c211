// A whole residual MLP (the Lorenz LOCAL score kernel: ScoreNet / ResMLP, sda/nn.py:31-71, sda/score.py:38-63 -- the network of four of
// the five checkpoints of experiments/lorenz/eval.py:33-39) in ONE launch, and its input VJP in one more.  The per-layer path
// (linear.hip: sda_linear / sda_row_ln) was ~20 launches forward + ~20 backward per score evaluation, each a separate pass over
// (rows x 128) activations in HBM.  Rows are independent (LayerNorm is over a row's features), so:
//   * a wave owns 16 ROWS and ALL features of them ("row private"): v_mfma_f32_16x16x4_f32 with D = [feature 16][row 16], eight D
//     fragments = 128 features of the wave's rows in 32 registers.  The K index of a fragment step is a free permutation as long as
//     both operands agree: with k(kq, s) = 16 (s >> 2) + 4 kq + (s & 3) the B operand of step s IS register (s >> 2)[s & 3] of the
//     previous layer's D fragments -- a layer's output feeds the next layer's multiply as it stands: no activation exchange through
//     LDS, no tile stores, no barrier between a GEMM and the next one's input.  (The first version gave a wave 32 output features of a
//     64-row tile: every layer boundary was registers -> LDS -> barrier -> LDS reads, LayerNorm crossed the four waves through LDS,
//     the narrow last layers ran on one wave -- 0.43 of the matrix peak, and a second workgroup per CU does not hide vector-ALU phases
//     under an fp32 MFMA stream: it owns the SIMD's VALU.)
//   * the weights are the A operands: per GEMM one slab [fragment m][k quad sq][lane][4] (element e of lane (kq, li) =
//     W[16 m + li][16 sq + 4 kq + e]; + the bias) staged in LDS -- 64.5 KiB for a 128 x 128 layer, two buffers: the next GEMM's slab is
//     copied (16-byte loads -> 16-byte LDS stores, no vector ALU) in pieces between the current one's multiplies; lanes read A
//     fragments lane-linearly (conflict free), one 16-byte read per four MFMAs; ONE workgroup barrier per GEMM (slab hand-off);
//   * LayerNorm is wave private: a row's 128 features sit in 4 lanes x 32 registers -- lane-local sums + two shuffles;
//   * saved for the VJP (16-byte stores): block inputs, pre-activations, mean / rstd -- as the per-layer path saved.
// Widths are padded: outputs to 16 / 128 / 256 features, contraction lengths to 16 / 64 / 128 / 256.
// Wide nets (a GEMM side in 129 .. 256: the reference's TRAINED local nets are 256 wide, experiments/lorenz/train.py:30-44) run the
// mlp_fwd_kernel_wide / mlp_bwd_kernel_wide kernels at the end of this file; nets whose GEMMs are all <= 128 run the kernels above them.
// Both sets call ONE copy of the multiply (ml_mm), the LayerNorm and its adjoint (ml_ln, ml_ln_bwd) and window mode's fold epilogue
// (ml_win_fold); window mode's two loaders exist twice (see ml_win_load).  The plan:
//   * still row private, 16 rows x ALL 256 features per wave: sixteen D fragments = 64 registers per activation array, and a GEMM's D
//     fragments are still the next GEMM's B operands as they stand.  LayerNorm: 4 lanes x 64 registers, the same two passes + two shuffles;
//   * a wide GEMM is streamed through LDS as UNITS: a side above 128 pads to 256 and splits in two halves of 128, so a 256 x 256 layer is
//     four ordinary 128 x 128 slabs, in memory in the order [output half][input half]; the second input half accumulates on the first
//     (its C operand is the accumulator).  Units pass through the two slab buffers exactly as whole GEMMs do above: unit u multiplies
//     (ml_mm, shared with the narrow kernels) while unit u + 1 is copied into the other buffer.  ONE barrier per unit: four per
//     256 x 256 GEMM, i.e. still one per 256 MFMAs of a wave;
//   * registers (one wave per SIMD: 512, architectural + accumulation unified on gfx950): forward a (residual stream), h (GEMM input),
//     acc = 192, + 64 of A fragments (ml_mm's double buffer) + 16-32 staging; VJP gacc, h, acc likewise.  What differs from the narrow
//     kernels to stay inside the file: the bias is added from LDS behind the GEMM (not 32 registers of C operand under the first
//     MFMAs), both saved streams are stored behind the block's first GEMM (no copy of z rides the second), the VJP reads the saved
//     streams behind the multiply, the pre-activations in groups of four fragments.  Compiled: no spill, no scratch instruction
//     (tests/test_isa_guard_mlp.py holds that);
//   * LDS: 2 x 64 KiB unit buffers + 16 KiB of biases = 144 KiB of 160, as the narrow kernels.  The bias region holds every GEMM's
//     padded bias: sixteen 256-wide GEMMs; beyond that SDA_E_UNSUPPORTED.
// Window mode (sda_mlp_fwd_win / sda_mlp_bwd_win, sda_hip.h) keeps a row's window values in the first one or two D fragments: windows of at most
// 16 values run the <true> instances of the four kernels, windows of 17 .. 32 values (Lorenz k = 3, 4) the mlp_win2_* kernels -- the same
// bodies (mlp1d_kernels.hpp, mlp1d_vjp_kernels.hpp) compiled with ML_WF = 2; the VJP's window gradient gwin has a row of 16 ML_WF floats.  A last GEMM of 17 .. 32
// outputs is a 128-feature slab, as every width above 16.
// Roofline: the Lorenz local net is 0.34 MFLOP per window and direction; at 62 464 windows (eval.py's batch) 21.5 GFLOP = 0.14 ms of
// fp32 MFMA time per direction.
#include "sda_common.hpp"
#include <stdlib.h>
#include <type_traits>

#ifdef SDA_ML_TRACE                    // tooling (tools/mlp_trace.py): per-phase cycle sums of workgroup 0 / wave 0, kept in scalar registers
__device__ long long ml_trace[16];     // and written once at the kernel's end (a stamp that touches memory drains the loads in flight)
#define ML_T0() long long ml_acc_[8] = {0, 0, 0, 0, 0, 0, 0, 0}; long long ml_tl = __builtin_readcyclecounter()
#define ML_STAMP(k) do { const long long n_ = __builtin_readcyclecounter(); ml_acc_[k] += n_ - ml_tl; ml_tl = n_; } while (0)
#define ML_DUMP() do { if (blockIdx.x == 0 && threadIdx.x == 0) for (int k_ = 0; k_ < 8; ++k_) ml_trace[k_] += ml_acc_[k_]; } while (0)
extern "C" int sda_ml_trace_read(long long* out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(ml_trace), sizeof(long long) * 16) != hipSuccess) return SDA_E_BADARG;
    if (reset) { long long z[16] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(ml_trace), z, sizeof(z)); }
    return SDA_OK;
}
#else
#define ML_T0() do {} while (0)
#define ML_STAMP(k) do {} while (0)
#define ML_DUMP() do {} while (0)
#endif
#include "mlp1d_common.hpp"

// ------------------------------------------------------------------------------------------------------------ the kernels
// {forward, VJP} x {rows, windows} x {narrow, wide}; window mode with the window values of a row in one D fragment (at most 16 values) ...
// (the VJP text's hooks, see mlp1d_vjp_kernels.hpp: both descriptors are parameters and no cotangent stream is stored)
#define ML_VJP_ARGS const sda_mlp_desc d, const sda_mlp_win w
#define ML_VJP_ENTRY
#define ML_COT(g, n, v) do {} while (0)
#define ML_WF 1
#define ML_K_FWD mlp_fwd_kernel
#define ML_K_BWD mlp_bwd_kernel
#define ML_K_FWD_WIDE mlp_fwd_kernel_wide
#define ML_K_BWD_WIDE mlp_bwd_kernel_wide
#include "mlp1d_kernels.hpp"
#include "mlp1d_vjp_kernels.hpp"
#undef ML_WF
#undef ML_K_FWD
#undef ML_K_BWD
#undef ML_K_FWD_WIDE
#undef ML_K_BWD_WIDE
// ... and in two (17 .. 32 values): only <true> of these is ever instantiated.  Kernels of their own rather than a run-time fragment count in
// the ones above, so that a window of at most 16 values runs the code it ran, bit for bit (tests/test_isa_guard_mlp_win2.py holds these to
// the same no-spill rule)
#define ML_WF 2
#define ML_K_FWD mlp_win2_fwd
#define ML_K_BWD mlp_win2_bwd
#define ML_K_FWD_WIDE mlp_win2_fwd_wide
#define ML_K_BWD_WIDE mlp_win2_bwd_wide
#include "mlp1d_kernels.hpp"
#include "mlp1d_vjp_kernels.hpp"
#undef ML_WF
#undef ML_K_FWD
#undef ML_K_BWD
#undef ML_K_FWD_WIDE
#undef ML_K_BWD_WIDE

// (*two: the window takes two D fragments -- the mlp_win2 kernels and a gwin row of 32 floats)
static int mlp_win_check(const sda_mlp_desc* d, const sda_mlp_win* w, bool bwd, bool* two) {
    if (!w || w->nw < 1 || w->c < 1 || w->len < w->nw || ((w->len - w->nw) & 1)) return SDA_E_BADARG;
    const int64_t wc64 = (int64_t)(w->len - w->nw + 1) * w->c;
    if (wc64 > 32) return SDA_E_UNSUPPORTED;               // (the window values of a row live in at most two D fragments)
    const int wc = (int)wc64;
    *two = wc > 16;
    if (d->rows % w->nw || !w->ghat || !w->coef) return SDA_E_BADARG;
    if (d->out_f[d->ngemm - 1] != wc) return SDA_E_BADARG;
    if (!bwd) {
        if (!w->x || !w->eps || !w->y || w->emb_n < 0 || (w->emb_n > 0 && !w->emb) || d->in_f[0] != wc + w->emb_n) return SDA_E_BADARG;
        if (w->p_step < 1 || w->c_step < 1 || w->p_start < 0 || w->c_start < 0 || w->p_stop > w->len || w->c_stop > w->c ||
            w->p_stop <= w->p_start || w->c_stop <= w->c_start)
            return SDA_E_BADARG;
    } else {
        if (!w->gwin || (reinterpret_cast<uintptr_t>(w->gwin) & 15) || d->in_f[0] < wc) return SDA_E_BADARG;
    }
    return SDA_OK;
}

template <bool BWD, bool WIN>
static int mlp_launch(const sda_mlp_desc* d, const sda_mlp_win* w, hipStream_t stream) {
    bool wide = false, two = false;
    int rc = mlp_check(d, BWD, WIN, &wide);
    if (rc != SDA_OK) return rc;
    if (WIN && (rc = mlp_win_check(d, w, BWD, &two)) != SDA_OK) return rc;
    const int64_t tiles = ((int64_t)d->rows + 63) / 64;
    if (tiles > 0x7fffffffLL) return SDA_E_UNSUPPORTED;
    constexpr int lds = (2 * ML_SLAB + ML_BIAS) * 4;
    static bool raised[4][SDA_MAX_DEVICES];
    // (the two-fragment kernels are named first: instantiated in that order, the object's last function stays mlp_fwd_kernel<true>, whose pinned
    // instruction count -- tests/test_isa_guard_mlp.py -- has no alignment padding behind it)
    void (*kern)(sda_mlp_desc, sda_mlp_win) = nullptr;
    if constexpr (WIN) {
        if (two) kern = wide ? (BWD ? mlp_win2_bwd_wide<true> : mlp_win2_fwd_wide<true>) : (BWD ? mlp_win2_bwd<true> : mlp_win2_fwd<true>);
    }
    if (!kern) kern = wide ? (BWD ? mlp_bwd_kernel_wide<WIN> : mlp_fwd_kernel_wide<WIN>) : (BWD ? mlp_bwd_kernel<WIN> : mlp_fwd_kernel<WIN>);
    const int rr = sda_raise_dyn_lds(reinterpret_cast<const void*>(kern), lds, raised[2 * two + wide]);
    if (rr != SDA_OK) return rr;
    sda_mlp_win wv = {};
    if (WIN) wv = *w;
#ifdef SDA_ML_TRACE
    sda_mlp_desc dd = *d;
    if (!BWD && getenv("SDA_ML_DBG")) {                     // tooling: which save stream costs what (results of a later VJP are wrong)
        const int b = atoi(getenv("SDA_ML_DBG"));
        if (b & 1) dd.a_save = nullptr;
        if (b & 2) dd.z_save = nullptr;
        if (b & 4) { dd.mean_save = nullptr; dd.rstd_save = nullptr; }
    }
    d = &dd;
#endif
    hipLaunchKernelGGL(kern, dim3((unsigned)tiles), dim3(256), lds, stream, *d, wv);
    return sda_launch_status();
}

extern "C" int sda_mlp_fwd(const sda_mlp_desc* d, void* stream) { return mlp_launch<false, false>(d, nullptr, (hipStream_t)stream); }
extern "C" int sda_mlp_bwd(const sda_mlp_desc* d, void* stream) { return mlp_launch<true, false>(d, nullptr, (hipStream_t)stream); }
extern "C" int sda_mlp_fwd_win(const sda_mlp_desc* d, const sda_mlp_win* w, void* stream) { return mlp_launch<false, true>(d, w, (hipStream_t)stream); }
extern "C" int sda_mlp_bwd_win(const sda_mlp_desc* d, const sda_mlp_win* w, void* stream) { return mlp_launch<true, true>(d, w, (hipStream_t)stream); }
// floats of GEMM (in_f -> out_f)'s slab, for the packer
extern "C" int sda_mlp_slab_floats(int in_f, int out_f) {
    if (in_f < 1 || out_f < 1 || in_f > 256 || out_f > 256) return SDA_E_UNSUPPORTED;
    return mlw_slab_floats(in_f, out_f);
}
