// A whole single-level 1-D U-Net (the Lorenz score networks of experiments/lorenz/utils.py:26-42: head convolution, the
// descent + ascent modulated residual blocks of sda/nn.py:18-28, tail convolution -- sda/nn.py:184-206 with one level) in ONE
// launch, and its input VJP in one more.  The per-block kernels of block1d.hip left a network evaluation at 8 launches
// forward + 8 backward, each ~60 % launch latency + first global round trip; here the dependency between layers stays inside a
// workgroup:
//   * a workgroup owns TP consecutive positions of one sequence and computes every layer on NC = 16 NF columns = TP + a halo
//     of H = (number of convolutions) positions per side.  A k = 3 convolution makes one more column per side depend on data
//     beyond the tile, so after all H convolutions exactly the TP own columns are exact; the halo columns are recomputed by
//     the neighbouring workgroups (1.8x redundant multiplies at NF = 4 -- the nets are latency-bound, not MFMA-bound).
//     Positions outside the sequence are forced to zero at every convolution input (zero padding) or wrap (circular).
//   * wave w owns output channels 16 w .. 16 w + 15 of every convolution (v_mfma_f32_16x16x4_f32; A = weight fragments held
//     in registers, B from LDS).  Every convolution's weights are packed [tap][64][64] (zero padded) in EXECUTION order in one
//     buffer, so a fragment load is one lane offset + a scalar offset; the weights of convolution i + 1 are loaded (L2 ->
//     registers, 48 dwords per lane) while convolution i multiplies: two register sets, alternating.  Biases and modulation
//     vectors are staged in LDS once per launch.
//   * the residual stream lives in registers in MFMA D layout (channel 16 w + 4 kq + r, column 16 nf + li) between layers;
//     LayerNorm statistics are reduced lane-locally, across the four lane groups (shuffles), across the four waves (LDS).
//   * what the VJP needs (block inputs a, pre-activations z, mean / rstd per position) is written for the own columns only;
//     the backward kernel reads it for its halo columns too (written by the neighbours' forward).
//   * input / output are addressed through (image, channel, position) strides: the (B, L, C) <-> (B, C, L) transposes of
//     MCScoreWrapper (sda/score.py:104-110) cost nothing on either side.
//   * whole-sequence tiles (round 4): with zero padding a tile that holds an ENTIRE sequence needs no halo at all -- what lies beyond
//     its edge columns is the padding itself.  When every sequence fits 16 NF <= 80 columns and there are enough sequences to fill the
//     chip (the reference's evaluation job: 1024 trajectories of 65 positions, experiments/lorenz/eval.py:72-84) a workgroup takes one
//     whole sequence: 80 columns per sequence instead of two 64-column tiles (1.8x halo recompute), nothing narrowed (`whole`).
//   * the validity cone (round 4): convolution i (0 = first of the launch) is only exact -- and only needed -- on columns
//     [1 + i, NC - 1 - i).  The 16-column MFMA fragments are therefore mapped so that the LAST one holds the tile's outermost
//     columns [0, 8) + [NC - 8, NC) (fragment nf < NF - 1 holds columns 8 + 16 nf ..): from convolution 7 on nothing in it is needed
//     any more, and the rest of the launch multiplies, normalises and stores NF - 1 fragments (7 of 14 convolutions of the Lorenz
//     nets: -25 % of the MFMAs at NF = 2, -12.5 % at NF = 4).  A stage may only drop the fragment once the stage feeding it wrote
//     nothing the next one reads there: a block's LayerNorm / residual store goes narrow one block later than its convolutions.
#include "sda_common.hpp"

#ifdef SDA_N1_TRACE                    // tooling (tools/net1d_trace.py): per-phase cycle sums of workgroup 0 / wave 0
__device__ long long n1_trace[16];
#define N1_T0() long long n1_tl = __builtin_readcyclecounter()
#define N1_STAMP(k) do { if (blockIdx.x == 0 && threadIdx.x == 0) { const long long n_ = __builtin_readcyclecounter(); n1_trace[k] += n_ - n1_tl; n1_tl = n_; } } while (0)
extern "C" int sda_n1_trace_read(long long* out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(n1_trace), sizeof(long long) * 16) != hipSuccess) return SDA_E_BADARG;
    if (reset) { long long z[16] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(n1_trace), z, sizeof(z)); }
    return SDA_OK;
}
#endif
#include "net1d.hpp"

template <bool BWD, int NF, bool FUSED>
static void net1d_launch_nf(const sda_net1d_desc* d, const sda_net1d_fuse& f, dim3 grid, int ptiles, int tp, int whole, hipStream_t stream) {
    if (BWD) hipLaunchKernelGGL((net1d_bwd_kernel<NF, FUSED>), grid, dim3(256), 0, stream, *d, f, ptiles, tp, whole);
    else hipLaunchKernelGGL((net1d_fwd_kernel<NF, FUSED>), grid, dim3(256), 0, stream, *d, f, ptiles, tp, whole);
}

template <bool BWD, bool FUSED>
static int net1d_launch(const sda_net1d_desc* d, const sda_net1d_fuse* fu, hipStream_t stream) {
    const int rc = net1d_check(d, BWD);
    if (rc != SDA_OK) return rc;
    int tp, ptiles, whole;
    const int nf = net1d_tiling(d, &tp, &ptiles, &whole);
    if (!nf) return SDA_E_UNSUPPORTED;
    if ((int64_t)d->n * ptiles > 0x7fffffffLL) return SDA_E_UNSUPPORTED;
    sda_net1d_fuse f = {};
    if (FUSED) {
        f = *fu;
        if (!f.coef) return SDA_E_BADARG;
        // eps / ghat / out / x share ONE layout (the output strides); the fused epilogues address all of them with it
        if (d->x_sn != d->out_sn || d->x_sc != d->out_sc || d->x_sx != d->out_sx || d->cin != d->cout) return SDA_E_BADARG;
        if (!BWD) {
            if (!f.y || !f.ghat || f.p_step < 1 || f.c_step < 1 || f.p_start < 0 || f.c_start < 0 || f.p_stop > d->len ||
                f.c_stop > d->cout || f.p_stop <= f.p_start || f.c_stop <= f.c_start)
                return SDA_E_BADARG;
        } else {
            if (!f.eps || f.mode < 0 || f.mode > 2 || (f.mode == 1 && (!f.xs || !f.step_coef)) ||
                (f.mode == 2 && (!f.partial || f.partial_stride < ptiles)))
                return SDA_E_BADARG;
            if (f.mode != 1) f.xs = d->out;                  // (never dereferenced; keeps the pointer arithmetic defined)
        }
    }
    const dim3 grid((unsigned)(d->n * ptiles));
    switch (nf) {
        case 2: net1d_launch_nf<BWD, 2, FUSED>(d, f, grid, ptiles, tp, whole, stream); break;
        case 3: net1d_launch_nf<BWD, 3, FUSED>(d, f, grid, ptiles, tp, whole, stream); break;
        case 4: net1d_launch_nf<BWD, 4, FUSED>(d, f, grid, ptiles, tp, whole, stream); break;
        default: net1d_launch_nf<BWD, 5, FUSED>(d, f, grid, ptiles, tp, whole, stream); break;
    }
    return sda_launch_status();
}

extern "C" int sda_net1d_fwd(const sda_net1d_desc* d, void* stream) { return net1d_launch<false, false>(d, nullptr, (hipStream_t)stream); }
extern "C" int sda_net1d_bwd(const sda_net1d_desc* d, void* stream) { return net1d_launch<true, false>(d, nullptr, (hipStream_t)stream); }
extern "C" int sda_net1d_fwd_fused(const sda_net1d_desc* d, const sda_net1d_fuse* f, void* stream) {
    if (!f) return SDA_E_BADARG;
    return net1d_launch<false, true>(d, f, (hipStream_t)stream);
}
extern "C" int sda_net1d_bwd_fused(const sda_net1d_desc* d, const sda_net1d_fuse* f, void* stream) {
    if (!f) return SDA_E_BADARG;
    return net1d_launch<true, true>(d, f, (hipStream_t)stream);
}
// tiles per sequence of the launch that would serve `d` (the row length of the fused backward's partial sums), <= 0: unsupported
extern "C" int sda_net1d_tiles(const sda_net1d_desc* d) {
    if (!d || d->len < 1 || d->nblocks < 0 || d->nblocks > SDA_NET1D_MAXB) return SDA_E_UNSUPPORTED;
    int tp, ptiles, whole;
    return net1d_tiling(d, &tp, &ptiles, &whole) ? ptiles : SDA_E_UNSUPPORTED;
}
