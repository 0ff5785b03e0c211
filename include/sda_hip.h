/*
 * sda_hip.h -- C ABI of libsda_hip.so: the MI355X (gfx950) kernels behind the
 * posterior-sampling hot path of francois-rozet/sda.
 *
 * The reference has no FFI/plugin boundary of its own (it is pure Python on
 * torch/ATen); its boundary is the nn.Module call protocol of sda/score.py and
 * sda/nn.py.  Each entry point below therefore names the reference arithmetic
 * (file:line under /root/reference) that it replaces.  The Python host side
 * (sda_amd/score.py, sda_amd/nn.py) keeps the reference's class names, call
 * signatures and state_dict keys and binds these symbols with ctypes
 * (sda_amd/_lib.py); INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 unless stated otherwise
 *   - strides are in ELEMENTS
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it,
 *     nothing synchronises, nothing allocates => every call is hipGraph-capturable
 *   - return value: 0 on success, <0 = SDA_E_* (argument/shape not supported),
 *     >0 = a hipError_t from the launch
 *   - internal activations are PLANAR: [n][c][h][w] contiguous (1-D nets: h = 1)
 */
#ifndef SDA_HIP_H
#define SDA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDA_ABI_VERSION 14

enum {
    SDA_OK = 0,
    SDA_E_BADARG = -1,      /* null pointer / non-positive size               */
    SDA_E_UNSUPPORTED = -2, /* shape outside what the gfx950 kernels tile     */
    SDA_E_LDS = -3          /* tile does not fit the 160 KiB LDS budget        */
};

/* activation ids: sda/utils.py:19-25 (ACTIVATIONS) */
enum { SDA_ACT_NONE = 0, SDA_ACT_SILU = 1, SDA_ACT_RELU = 2, SDA_ACT_ELU = 3, SDA_ACT_GELU = 4, SDA_ACT_SELU = 5 };

int sda_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution on the fp32 matrix cores (v_mfma_f32_32x32x2_f32).
 *
 * Replaces nn.Conv1d/nn.Conv2d as used by sda/nn.py:113-129,131-142,148-176 (heads, tails,
 * residue convs; padding = k//2; padding_mode zeros|circular; stride 1|2), and -- with
 * transposed/flipped packed weights -- their backward-data (what torch.autograd.grad computes
 * through them at sda/score.py:394).  Fused into the input loader (so no tensor is
 * materialised for them):
 *   - the sliding-window view of MCScoreNet.unfold           (sda/score.py:146-153)  [two-level batch stride]
 *   - the broadcast context/forcing channel concat           (sda/score.py:87, experiments/kolmogorov/utils.py:45-46)
 *   - the time modulation add + zuko LayerNorm over channels (sda/nn.py:28,137,163)   [mod, ln_mean, ln_rstd]
 *   - the activation between the two residue convs           (sda/nn.py:139)          [act_in]
 *   - nn.Upsample(nearest) before the tail conv              (sda/nn.py:164)          [up]
 *   - zero insertion (transposed stride-2 conv, backward of sda/nn.py:152-159)        [zins]
 * Fused into the epilogue: bias, multiply by act'(z) (backward through sda/nn.py:139),
 * residual/skip add (sda/nn.py:28,202).
 *
 * out[n][co][oy][ox] = bias[co] + sum_{ci,dy,dx} W[dy*kw+dx][ci][co] * V(n, ci, oy*stride_h+dy-kh/2, ox*stride_w+dx-kw/2)
 * V = virtual input: source x (and ctx channels) after  +mod -> LN -> act_in,  seen through
 *     nearest-upsample `up` or zero-insertion `zins`, padded circularly or with zeros.
 * ------------------------------------------------------------------------------------------ */
typedef struct sda_conv_desc {
    /* source tensor */
    const float* x;
    int64_t x_sn_outer, x_sn_inner; /* image n -> with m = n + x_n_off: (m / n_inner) * sn_outer + (m % n_inner) * sn_inner */
    int32_t n_inner;                /* >=1; windows per trajectory for the unfold view, else 1 (use sn_inner=0) */
    int32_t x_n_off;                /* image index offset applied before the n -> address map (chunked execution) */
    int64_t x_sc, x_sy, x_sx;       /* channel / row / column strides */
    int32_t cx;                     /* channels taken from x */
    const float* ctx;               /* optional extra channels appended after cx: planar [cctx][hs][ws] */
    int64_t ctx_sn;                 /* batch stride of ctx (0 = broadcast over n) */
    int32_t cctx;
    int32_t n;                      /* number of images */
    int32_t hs, ws;                 /* source spatial size */
    int32_t up_h, up_w;             /* >=1  nearest upsample of the source, per axis (1-D nets: up_h = 1) */
    int32_t zins_h, zins_w;         /* >=1  zero insertion (virtual[y][x] = src[y/zh][x/zw] iff both divisible) */
    /* loader transforms (all optional) */
    const float* mod;               /* [*][cx] additive per-channel modulation */
    int64_t mod_sn;                 /* per-image stride of mod (0 = shared) */
    const float* ln_mean;           /* [n][hs*ws] channel-LayerNorm statistics of (x + mod) */
    const float* ln_rstd;
    int32_t act_in;                 /* SDA_ACT_* applied after LN */
    /* filter */
    int32_t kh, kw, stride_h, stride_w, circular;
    const float* w;                 /* packed [kh*kw][cin_pad][cout_pad], see sda_pack_conv_weight */
    int32_t cin_pad, cout_pad;
    const float* bias;              /* [cout] or NULL */
    /* output: planar contiguous [n][cout][ho][wo] */
    float* out;
    int32_t cout, ho, wo;
    /* epilogue (tensors shaped like out) */
    const float* dact_z;            /* out *= act'(dact_z)  (NULL = off) */
    int32_t act_d;
    const float* res;               /* out += res           (NULL = off) */
    /* tiling: cout tile = 32*mt (mt in 1..4); weights must be packed with cout_pad % (32*mt) == 0 */
    int32_t mt;
    /* optional overrides (all zero = the defaults above, so a zero-initialised descriptor keeps its meaning).
     *   explicit_pad != 0: taps read in[o*stride + t - pad_h|pad_w]; default kh/2, kw/2 (odd kernels).  Even kernels
     *   need it.
     *   out_sn / out_sc / out_sy / out_sx: element strides of `out` (and of dact_z / res, which always share its
     *   layout) per image / channel / row / pixel; all zero = planar contiguous.  With pad they let the VJP of a
     *   stride-2 convolution run as one small stride-1 convolution per output parity class, each writing its own
     *   interleaved quarter of the gradient, instead of convolving a zero-inserted tensor (4x the multiplies). */
    int32_t explicit_pad, pad_h, pad_w;
    int64_t out_sn, out_sc, out_sy, out_sx;
    /* optional Winograd F(2x2,3x3) weights (sda_pack_conv_weight_wino4: [cin_pad/8][16][cout/16][64][2], U fragments in MFMA lane
     * order): 2.25x fewer multiplies than the direct kernel, fp32 round-off-level error.  When non-NULL the Winograd kernel
     * (csrc/conv_wino4.hip) takes the launch if ALL of this holds, and the direct kernels serve it otherwise:
     *   3 x 3, stride 1, no zero insertion, default padding and planar output (explicit_pad and out_s* zero);
     *   cout % 32 == 0 and cout_pad == cout: the cout tile is 96 where cout % 96 == 0 (the reference's training widths), else 64
     *     where cout % 64 == 0 (its default widths (64, 128, 256), experiments/kolmogorov/utils.py:52), else 32 (sda/nn.py:99);
     *   output height a multiple of 8 and width of 16 (workgroup tile = 16 x 8 pixels of one image), source up-sampled by 1 or 2;
     *   loader fusions none / SiLU / LayerNorm / modulation (shared by all images) + LayerNorm; ctx channels only without any.
     * SDA_CONV_WINO=0 or SDA_CONV_WINO4=0 in the environment switch the kernel off.  (The first-generation kernel and its weight field, ABI <= 13,
     * are retired: even-sized images that do not tile by 8 x 16 and other activations now run direct.) */
    const float* w_wino4;
    /* optional output pooling (0 / 1 = off): out is [n][cout][ho / pool_h][wo / pool_w] and receives the SUM of each pool_h x pool_w
     * cell of the convolution's ho x wo output -- the input VJP of `Upsample(nearest) -> conv` (the tails, sda/nn.py:161-169) in one
     * launch, without the full-resolution gradient in between.  Served for (2, 2) by the w_wino4 kernel on plain launches (no loader
     * fusion, no epilogue operand): 7 of the 16 Winograd positions have weight zero in the cell sum and are never multiplied.
     * Anything else: SDA_E_UNSUPPORTED (run the plain launch and pool in the reader, sda_ln_bwd's pool arguments). */
    int32_t pool_h, pool_w;
    /* optional (may be NULL): the w_wino4 weights re-packed for the zero-position kernels (sda_pack_conv_weight_wino4_zp) -- per
     * (K stage, cout tile) the 9 live Winograd positions only, 28 KiB instead of the 36 KiB of the six position pairs that hold
     * them (96-cout tile; 20 / 12 KiB for the 64- / 32-cout tiles).  With it the 2 x 2 up-sampled / pooled launches above run their zero-position form; without it the up-sampled launch
     * runs the full kernel (same result bit for bit) and the pooled launch is SDA_E_UNSUPPORTED. */
    const float* w_wino4_zp;
    /* OPT-IN (ABI v11; all zero = off): the fp32 multiply emulated on the f16 matrix cores, fp32 accumulation (csrc/conv_h2.hip).
     *   w_h2: sda_pack_conv_weight_h2's packing of the layer (every weight as two halves hi + lo of s_w w), w_h2_scale = s_w
     *         (sda_conv_h2_scale(max |w|)).
     *   x_amax: device scalar, max |value the loader feeds the multiply| (after modulation + LayerNorm / activation) or any upper
     *         bound of it -- sda_absmax of the tensor, or the out_amax of the launch that produced it; NULL: x_amax_static (a bound
     *         known on the host: sqrt(channels) behind a LayerNorm).  The kernel derives the power-of-two input scale from it.
     *   out_amax: optional device scalar, atomically maxed (as uint bits; the caller zeroes it) with max |out| of this launch.
     * Also served, with their own packings in w_h2 (see sda_pack_conv_weight_h2_up / _rows below): up_h = up_w = 2 (the tails), pool_h =
     * pool_w = 2 (their VJP summed over the cells), stride_h = stride_w = 2 (the level heads; w_h2 = the four parity classes'
     * sda_pack_conv_weight_h2_rows packings back to back, class (py, px) = taps dy in ((1), (0, 2))[py] x dx alike, rows = cout, k = cin),
     * zins_h = zins_w = 2 (the heads' input VJP: the same with rows = forward cin, k = forward cout).
     * Served by sda_conv_h2 for 3 x 3 / stride 1 / cin % 32 == 0 / cout % 96 == 0 or cout % 64 == 0 (ABI v13; % 96 both before) / 16 x 16-tileable planar launches with the loader
     * fusions none / activation / (modulation +) LayerNorm and the epilogues bias, x act'(z), + res; sda_conv_igemm ignores the
     * fields.  Error against float64 equals the fp32 Winograd kernel's (3e-7, tools/f16_split_numerics.py). */
    const void* w_h2;
    float w_h2_scale;
    float x_amax_static;
    const float* x_amax;
    float* out_amax;
} sda_conv_desc;

int sda_conv_igemm(const sda_conv_desc* d, void* stream);
/* Backward-data of a stride-2 3 x 3 convolution (the gradient through the level heads, sda/nn.py:152-159) as ONE launch: the four
 * output parity classes of the split formulation above together.  d = the class-(0,0) launch (kh = kw = 2, explicit_pad with pad 0,
 * out / res = the class-(0,0) strided views of the planar [n][cout][2 ho][2 wo] gradient / skip tensors) with d->w = the four
 * classes' sda_pack_conv_weight packings (transpose = 1) back to back in the order (0,0), (0,1), (1,0), (1,1): [9][cin_pad][cout_pad].
 * SDA_E_UNSUPPORTED outside the kernel's range (cout % 32 -- 96- / 64- / 32-cout tiles as sda_conv_desc.w_wino4 --, ho % 8, wo % 16,
 * loader fusions): run the four class launches. */
int sda_conv_parity4(const sda_conv_desc* d, void* stream);
/* which kernel family would serve the launch (pure planning, nothing is launched): 0 = direct implicit GEMM, 2 = the Winograd
 * kernel (w_wino4), 5 = the same in its zero-position form (2 x 2 up-sampled source or pooled output: 54 of the 96 multiplies
 * per stage), 3 = the single-round-trip small 1-D kernel, 4 = the 3 x 3 kernel for <= 16 output channels; <0 error.
 * (1 was the first-generation Winograd kernel: retired, never returned.) */
int sda_conv_igemm_path(const sda_conv_desc* d);
/* positions per workgroup (16, 32 or 64) of the small 1-D kernel's launch where sda_conv_igemm_path(d) is 3: 16 while
 * n * ceil(wo / 16) <= 1024, else 32 while n * ceil(wo / 32) <= 1024, else 64 (SDA_SMALL1D_TP=16|32|64 in the environment forces
 * one); 0 where that kernel does not take the launch (more than 4096 workgroups among the reasons); SDA_E_BADARG for ln_mean
 * without ln_rstd.  Host only, nothing is launched; x, w, out and the ln_* pointers are tested for NULL, never dereferenced. */
int sda_small1d_tile(const sda_conv_desc* d);
/* bytes of dynamic LDS the launch would use (or <0 error), for planning / tests */
int64_t sda_conv_igemm_lds_bytes(const sda_conv_desc* d);

/* ------------------------------------------------------------------------------------------
 * Parameter gradients of the convolutions (csrc/conv_wgrad.hip).  Additions that keep ABI v13: no existing entry or struct
 * changes.  They replace what torch.autograd forms for the weights and biases of sda/nn.py:113-176's nn.Conv1d / nn.Conv2d when
 * the reference trains (sda/score.py:265-276 ``loss`` -> ``backward()``, driven by sda/utils.py:89-165 ``loop``):
 *
 *   dw[co][ci][ky][kx] (+)= sum_{n,oy,ox} g[n][co][oy][ox] * V(n, ci, oy*stride_h + ky - pad_h, ox*stride_w + kx - pad_w)
 *   db[co]             (+)= sum_{n,oy,ox} g[n][co][oy][ox]
 *
 * V is the layer's input as its FORWARD launch read it: `conv` is that launch's descriptor (source view incl. the sliding-window
 * and context channels, mod / ln_mean / ln_rstd / act_in, up-sampling, stride, padding, kh / kw, cout, ho / wo); its w, bias, out,
 * dact_z, res, mt and Winograd / f16 fields are ignored, zins and pool must be off.  g: the cotangent at the convolution's output,
 * planar contiguous [n][cout][ho][wo].  dw: torch layout [cout][cin][kh][kw] (cin = cx + cctx), db: [cout] or NULL.
 * The contraction over positions is cut into `slabs` ranges (0 = planner's choice, a function of the shape; at most 64) whose
 * partial results go to `work` (sda_conv_wgrad_work_floats floats) and are summed in slab order by a second kernel: no atomics,
 * bitwise reproducible.  accumulate = 1 adds into dw / db (chunks of the image axis), 0 overwrites.
 * ------------------------------------------------------------------------------------------ */
typedef struct sda_wgrad_desc {
    sda_conv_desc conv;
    const float* g;
    float* dw;
    float* db;
    float* work;
    int32_t slabs;
    int32_t accumulate;
} sda_wgrad_desc;

int sda_conv_wgrad(const sda_wgrad_desc* d, void* stream);
/* planning only (nothing is launched): the slab count the launch would use / the floats of `work` it needs; <0 error */
int sda_conv_wgrad_slabs(const sda_wgrad_desc* d);
int64_t sda_conv_wgrad_work_floats(const sda_wgrad_desc* d);
/* OPT-IN second route for the 3 x 3 block convolutions (csrc/conv_wgrad3.hip; additions that keep ABI v14).  Same descriptor, same
 * result layout, same slab-order reduction (no atomics, bitwise reproducible, `accumulate` as above); the input tile is staged once
 * with its halo and the nine taps are shifted reads of it.  Served: 2-D, kh = kw = 3, stride 1, up = zins = pool = 1, cctx = 0, no
 * explicit pad, planar contiguous source (x_sx = 1, x_sy = ws, x_sc = hs * ws, n_inner = 1), cx % 32 == 0, cout % 32 == 0, circular or
 * zero padding, loader = ln_mean / ln_rstd + mod (conv1), act_in (conv2) or none, a tile within the 160 KiB LDS (ws <= ~180).
 * `slabs`: 0 = planner's choice (a function of the shape), at most 256; `work` holds sda_conv_wgrad3_work_floats floats.
 *   sda_conv_wgrad3_serves: 1 when the launch is in the served set, else 0 (planning only, nothing is launched)
 *   sda_conv_wgrad3: SDA_E_UNSUPPORTED outside the served set (run sda_conv_wgrad) */
int sda_conv_wgrad3_serves(const sda_wgrad_desc* d);
int64_t sda_conv_wgrad3_work_floats(const sda_wgrad_desc* d);
int sda_conv_wgrad3(const sda_wgrad_desc* d, void* stream);
/* OPT-IN tiled route for the stride-2 heads and up-sampling tails (csrc/conv_wgrad3.hip, the same kernel template; additions that
 * keep ABI v14): the design, descriptor, result layout, slab range and reduction of sda_conv_wgrad3 for two more geometries.  Served: as sda_conv_wgrad3 but
 *   up2: up_h = up_w = 2, stride 1, ho = 2 hs, wo = 2 ws, loader = ln_mean / ln_rstd alone (no mod, no act_in) or none;
 *   s2:  stride_h = stride_w = 2, up = 1, hs and ws even, ho = hs / 2, wo = ws / 2, plain loader (no ln, mod, act_in);
 * a tile within the 160 KiB LDS.  `work` holds sda_conv_wgrad3x_work_floats floats.
 *   sda_conv_wgrad3x_serves: 1 when the launch is in the served set, else 0 (planning only, nothing is launched)
 *   sda_conv_wgrad3x: SDA_E_UNSUPPORTED outside the served set (run sda_conv_wgrad3 or sda_conv_wgrad) */
int sda_conv_wgrad3x_serves(const sda_wgrad_desc* d);
int64_t sda_conv_wgrad3x_work_floats(const sda_wgrad_desc* d);
int sda_conv_wgrad3x(const sda_wgrad_desc* d, void* stream);
/* Gradient of the modulation rows (sda/nn.py:28 ``x + project(y)`` before the LayerNorm): spatial sums of the cotangent at the
 * LayerNorm's input.  x, y: planar [n][c][hw]; out[i * out_sn + ch] (+)= sum_pix (x - y)[i][ch][pix] (y = NULL: x alone), or
 * with sum_images = 1 (a time embedding shared by all images) out[ch] (+)= sum_i sum_pix, images summed in order.
 * accumulate = 1 adds into out.  Fixed-order reductions, no atomics. */
int sda_plane_sum(const float* x, const float* y, int n, int c, int64_t hw, float* out, int64_t out_sn, int sum_images,
                  int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------
 * One modulated residual block of a 1-D U-Net in ONE launch (sda/nn.py:18-28, 113-176 with spatial = 1):
 *     y = a + conv2(act(conv1(LN(a + mod)))),   both convolutions c -> c, kernel 3, stride 1, same padding mode;
 * and its input VJP  gx = g + LN^T(conv1^T(act'(z) . conv2^T(g))).  For the latency-bound nets of the Lorenz experiments
 * (c <= 64): three launches forward / three backward become one each.  a, y, z, g, gx: planar [n][c][len] contiguous;
 * mean / rstd: [n][len].  w1 / w2: sda_pack_conv_weight packings [3][k_pad][m_pad] -- FORWARD form for sda_block1d_fwd,
 * BACKWARD-DATA form (transpose = 1) for sda_block1d_bwd.  SDA_E_UNSUPPORTED when the shape is outside the kernel's range
 * (callers fall back to sda_ln_stats + sda_conv_igemm + sda_ln_bwd). */
typedef struct sda_block1d_desc {
    int32_t n, c, len;
    int32_t circular, act, unbiased;   /* padding mode of both convolutions; SDA_ACT_*; LayerNorm variance convention */
    float eps;
    int32_t k_pad, m_pad;
    const float* a;
    const float* mod;                  /* [*][c] additive modulation (NULL = none) */
    int64_t mod_sn;                    /* per-image stride of mod (0 = shared) */
    const float* w1; const float* b1;  /* b1 / b2 may be NULL; unused by the VJP */
    const float* w2; const float* b2;
    float* z;                          /* fwd: out (pre-activation of conv1, NULL = not kept); bwd: in */
    float* mean; float* rstd;          /* fwd: out (NULL = not kept); bwd: in */
    float* y;                          /* fwd: out */
    const float* g;                    /* bwd: in */
    float* gx;                         /* bwd: out */
} sda_block1d_desc;
int sda_block1d_fwd(const sda_block1d_desc* d, void* stream);
int sda_block1d_bwd(const sda_block1d_desc* d, void* stream);
/* positions per workgroup (16, 32 or 64) of the launch serving `d`, forward and VJP alike, or SDA_E_UNSUPPORTED
 * (host, no launch; reads the shape fields only, pointers may be NULL) */
int sda_block1d_tile(const sda_block1d_desc* d);

/* ------------------------------------------------------------------------------------------
 * A whole SINGLE-LEVEL 1-D U-Net in ONE launch (the Lorenz score networks, experiments/lorenz/utils.py:26-42;
 * sda/nn.py:184-206 with one level: head convolution cin -> c, `nblocks` modulated residual blocks (descent then ascent,
 * sda/nn.py:18-28), tail convolution c -> cout; every convolution kernel 3, stride 1, one padding mode), and its input VJP
 * in one more.  A workgroup owns a run of positions of one sequence and recomputes a halo of one position per convolution
 * and side (csrc/net1d.hip), so no layer ever waits for another workgroup.
 *   x / out: addressed as base + image * sn + channel * sc + position * sx (elements): (B, C, L) and (B, L, C) tensors alike.
 *   w: every convolution as an sda_pack_conv_weight packing [3][64][64] (k_pad = m_pad = 64: zero padded), 2 + 2 nblocks of them
 *   back to back in EXECUTION order; bias: [2 + 2 nblocks][64] zero padded, same order (NULL = none).
 *     sda_net1d_fwd: FORWARD packings: head, (conv1, conv2) of block 0 .. nblocks - 1, tail.
 *     sda_net1d_bwd: BACKWARD-DATA packings (transpose = 1): tail^T (cout -> c), (conv2^T, conv1^T) of block nblocks - 1 .. 0,
 *                    head^T (c -> cin); x = the incoming cotangent (cin = its channels), out = the input gradient (cout = its
 *                    channels); mod[k] is still the modulation of forward block k.
 *   a_save / z_save [nblocks][n][c][len], mean_save / rstd_save [nblocks][n][len] (block strides save_stride / stat_stride):
 *   written by the forward when non-NULL (all four or none), read by the VJP.
 * SDA_E_UNSUPPORTED outside the kernel's range (callers fall back to the per-block kernels). */
#define SDA_NET1D_MAXB 8
typedef struct sda_net1d_desc {
    int32_t n, len;
    int32_t cin, c, cout;
    int32_t nblocks;
    int32_t circular, act, unbiased;
    float eps;
    const float* x; int64_t x_sn, x_sc, x_sx;
    float* out; int64_t out_sn, out_sc, out_sx;
    const float* w;
    const float* bias;
    const float* mod[SDA_NET1D_MAXB];  /* [*][c] additive modulation of block k (NULL = none) */
    int64_t mod_sn;                    /* per-image stride of every mod (0 = shared) */
    float* a_save; float* z_save; int64_t save_stride;
    float* mean_save; float* rstd_save; int64_t stat_stride;
} sda_net1d_desc;
int sda_net1d_fwd(const sda_net1d_desc* d, void* stream);
int sda_net1d_bwd(const sda_net1d_desc* d, void* stream);

/* One Gaussian-guided score evaluation (GaussianScore.forward, sda/score.py:375-396) of such a network in TWO launches -- the
 * dependency minimum: every position of eps feeds the likelihood, whose cotangent feeds the VJP at every position -- and the
 * predictor / corrector bookkeeping of VPSDE.sample (sda/score.py:250-261) in their epilogues (ABI v7):
 *   sda_net1d_fwd_fused: out = eps = (cx0 + cx1 sigma) x + cn net(x, t) and
 *                        ghat = A^T((y - A x_hat) / (std^2 + gamma (sigma/mu)^2)), x_hat = (x - sigma eps) / mu   (score.py:387-392)
 *                        for A = x[..., p_start:p_stop:p_step, c_start:c_stop:c_step] (experiments/lorenz/eval.py:75), y
 *                        [n or 1][positions][channels] observed values;
 *   sda_net1d_bwd_fused: x = ghat; out = eps - (sigma/mu)(ghat - sigma J_eps^T ghat)   (score.py:394-396), then by `mode`
 *                        0: write out;  1: x <- r x + c1 out in place (score.py:252-253; out is not written);
 *                        2: write out and partial[image][tile] = sum of out^2 over the tile (score.py:259: delta = tau / mean(eps^2)).
 * (cx0, cx1, cn) = (0, 0, 1) is a bare network; other values serve estimators of the form eps = a(t) x + c net(x, t) (bench.py's
 * synthetic score).  x, eps, ghat, out share the (sn, sc, sx) strides of the descriptor's `out`; cin == cout.
 * coef: device {mu(t), sigma(t)}; step_coef: device {r, c1}.  Arithmetic = the unfused kernels' (same operations, same order). */
typedef struct sda_net1d_fuse {
    float cx0, cx1, cn;
    const float* coef;
    const float* y; int64_t y_sn;      /* fwd: observation; per-image stride (0 = one observation shared by the batch) */
    int32_t p_start, p_step, p_stop;   /* fwd: observed positions */
    int32_t c_start, c_step, c_stop;   /* fwd: observed channels */
    float std, gamma;
    float* ghat;                       /* fwd: out */
    const float* eps;                  /* bwd: in (the forward's out) */
    int32_t mode;                      /* bwd */
    float* xs;                         /* bwd mode 1: x, in place */
    const float* step_coef;            /* bwd mode 1 */
    float* partial; int32_t partial_stride;   /* bwd mode 2: [n][partial_stride >= sda_net1d_tiles(d)] */
} sda_net1d_fuse;
int sda_net1d_fwd_fused(const sda_net1d_desc* d, const sda_net1d_fuse* f, void* stream);
int sda_net1d_bwd_fused(const sda_net1d_desc* d, const sda_net1d_fuse* f, void* stream);
int sda_net1d_tiles(const sda_net1d_desc* d);          /* tiles per sequence of the launch serving `d` (host, no launch) */

/* Parameter gradients of such a network (opt-in training, sda_amd/training.py with net1d = True; csrc/net1d_train.hip; additive
 * to ABI v14).  A training step is one forward launch, three backward launches and, after the optimizer, one pack launch.
 *
 * sda_net1d_fwd_train: sda_net1d_fwd with saves -- the same out, a_save, z_save, mean_save, rstd_save bit for bit (all four saves
 *   are required when nblocks > 0) -- that also writes the tail convolution's input (the last block's output) to
 *   tail_in[n][c][len].  g_save / mod_part are not read.
 * sda_net1d_bwd_train: sda_net1d_bwd -- the same input gradient bit for bit -- that also stores the cotangent at every
 *   convolution's output as planes [n][c][len] in g_save, slot s at g_save + s * g_stride (g_stride >= n * c * len):
 *     s = 2 k: g at entry to block k (conv2's output cotangent);  s = 2 k + 1: q = conv2^T(g) act'(z) (conv1's);
 *     s = 2 nblocks: the stream cotangent in front of head^T (the head's).  The tail's output cotangent is net.x itself.
 *   and the modulation-row gradient of block k, sum over positions of rstd (gh - mean_c(gh) - xhat mean'_c(gh xhat)), as per-tile
 *   partial sums in the fixed slot mod_part[k][n][tile][c], tile < mod_tiles = sda_net1d_tiles(&net) (no atomics; every slot of a
 *   launch is written).  mod_part is required when nblocks > 0, g_save always; tail_in is not read. */
typedef struct sda_net1d_train_desc {
    sda_net1d_desc net;
    float* tail_in;
    float* g_save; int64_t g_stride;
    float* mod_part; int32_t mod_tiles;
} sda_net1d_train_desc;
int sda_net1d_fwd_train(const sda_net1d_train_desc* t, void* stream);
int sda_net1d_bwd_train(const sda_net1d_train_desc* t, void* stream);

/* sda_net1d_wgrad: the weight and bias gradients of all 2 + 2 nblocks convolutions in ONE launch on the fp32 matrix cores
 * (v_mfma_f32_16x16x4_f32) and ONE reduction launch behind it; bitwise reproducible.  For convolution v (FORWARD order: head,
 * (conv1, conv2) of block 0 .. nblocks - 1, tail)
 *     dw[v][co][ci][tap] = sum_{n, x} G[n][co][x] U[n][ci][x + tap - 1],   db[v][co] = sum_{n, x} G[n][co][x]
 * (x + tap - 1 outside the sequence: zero, or wrapped when net.circular) in torch's unpadded Conv1d layouts (cout, cin, 3) / (cout).
 * U is rebuilt from what sda_net1d_fwd_train saved -- head: net.x through (x_sn, x_sc, x_sx); conv1 of block k:
 * (a_k + mod_k - mean_k) rstd_k; conv2: act(z_k); tail: tail_in -- and G is read from g_save (see sda_net1d_bwd_train), the tail's
 * from gout through its strides.  The contraction axis (n len) is cut into `slabs` contiguous ranges (0: the planner's count, a
 * function of the shapes only; 1 .. 64 forces one, capped by the number of 32-row stages); workgroup (slab, convolution, column
 * tile) writes its unreduced 64 x 128 tile to work[sda_net1d_wgrad_work_floats(d)], the reduction sums the slabs in slab order.
 * It also finishes the modulation gradients: dmod[k][i * dmod_sn + ch] = sum over tiles (in tile order) of mod_part[k][i][tile][ch]
 * per image i when net.mod_sn != 0, or one row dmod[k][ch] summed over images in image order (tiles inside) when net.mod_sn == 0.
 * A NULL dw[v] / db[v] / dmod[k] skips that output (frozen parameters); nothing outside the unpadded extents is written.
 * Of `net`: the shapes, circular, act, x and its strides, mod / mod_sn, the four saves and their strides are read; w, bias, out are not.
 * Served: what sda_net1d_fwd serves, n len < 2^31.  SDA_E_UNSUPPORTED / SDA_E_BADARG as its siblings.
 * sda_net1d_wgrad_slabs / _work_floats: planning only (host): the slab count / the floats of `work` of that launch (< 0: error). */
typedef struct sda_net1d_wgrad_desc {
    sda_net1d_desc net;
    const float* tail_in;
    const float* g_save; int64_t g_stride;
    const float* gout; int64_t gout_sn, gout_sc, gout_sx;
    const float* mod_part; int32_t mod_tiles;
    float* dw[2 + 2 * SDA_NET1D_MAXB];
    float* db[2 + 2 * SDA_NET1D_MAXB];
    float* dmod[SDA_NET1D_MAXB]; int64_t dmod_sn;
    float* work;
    int32_t slabs;
} sda_net1d_wgrad_desc;
int sda_net1d_wgrad(const sda_net1d_wgrad_desc* d, void* stream);
int sda_net1d_wgrad_slabs(const sda_net1d_wgrad_desc* d);
int64_t sda_net1d_wgrad_work_floats(const sda_net1d_wgrad_desc* d);

/* sda_net1d_pack: every packing the whole-net kernels read, in ONE launch, from the 2 + 2 nblocks torch-layout weights (cout, cin, 3)
 * and biases (cout; NULL = none) given in FORWARD order (head cin -> c, the blocks' c -> c, tail c -> cout):
 *   wf:   the forward buffer of sda_net1d_fwd ([3][64][64] per convolution, forward order);
 *   wb:   the backward-data buffer of sda_net1d_bwd (transposed packings in its execution order; head^T keeps cin_keep input channels);
 *   bias: [2 + 2 nblocks][64] zero-padded rows, forward order.
 * A pure permutation: the bytes sda_pack_conv_weight (k_pad = m_pad = 64) and a bias copy produce.  NULL wf / wb / bias: not written. */
typedef struct sda_net1d_pack_desc {
    int32_t nblocks, cin, c, cout, cin_keep;
    const float* w[2 + 2 * SDA_NET1D_MAXB];
    const float* b[2 + 2 * SDA_NET1D_MAXB];
    float* wf; float* wb; float* bias;
} sda_net1d_pack_desc;
int sda_net1d_pack(const sda_net1d_pack_desc* p, void* stream);

/* Everything a predictor-corrector step needs before its score evaluations, in ONE launch (sda/score.py:250-253 scalars,
 * TimeEmbedding score.py:15-35, every block's `project` nn.py:132-135), for up to two time values:
 *   table != NULL: row = table[istep[0]] = {t, t - dt, r, c1, sigma(t - dt)} (the host-evaluated schedule of VPSDE.sample);
 *                  times = {t, t - dt};  istep[0] is incremented AFTER everything is written (single workgroup: the only reader);
 *   table == NULL: times = t_dev[0 .. nt).
 * out_coef (floats): {mu(t0), sigma(t0), mu(t1), sigma(t1), r, c1, sigma_next, t0, t1};  out_step (int64, optional): the step index
 * the row was read at;  mod: [nt][cp] modulation vectors -- or, with cp = 0 (wp NULL: a ScoreNet has no projections), the time
 * embedding itself, [nt][e].  Arithmetic identical to sda_vp_schedule / sda_time_embed /
 * sda_linear_small. */
int sda_step1d_prologue(const float* table, int row_len, int64_t* istep, const float* t_dev, int nt,
                        int alpha_kind, float eta, float k, int sigma_kind,
                        const float* freqs, int nf, const float* w0, const float* b0, int hidden, const float* w2, const float* b2, int e,
                        const float* wp, const float* bp, int cp,
                        float* out_coef, int64_t* out_step, float* mod, void* stream);
/* Which kernel sda_step1d_prologue launches for these sizes and weight addresses (host, no launch, nothing dereferenced): 1 = staged
 * (the three weight matrices copied into LDS first: power-of-two row lengths, 2 nf >= 8, 16-byte aligned matrices, at most 140 KiB and
 * 8192 16-byte loads), 0 = unstaged (rows read from global memory), or the SDA_E_* that sda_step1d_prologue returns for them. */
int sda_step1d_prologue_path(int nf, int hidden, int e, int cp, const float* w0, const float* w2, const float* wp);
/* sda_pc_correct with z = the row-keyed N(0, 1) draw of sda_randn_rows generated in the kernel (same Philox counters: identical
 * values), draw index = draw_dev[0] * draw_mul + draw_add  (sda/score.py:257-261). */
int sda_pc_correct_keyed(float* x, const float* eps, int b, int64_t per_sample, const float* partial, int nchunk, float tau,
                         float sigma, const float* coef_dev, uint64_t seed, int64_t row0, const int64_t* draw_dev, int64_t draw_mul,
                         int64_t draw_add, void* stream);

/* Repack torch-layout conv weights [cout][cin][kh][kw] for sda_conv_igemm.
 *   transpose = 0: forward          dst[tap][ci][co]        = w[co][ci][dy][dx]
 *   transpose = 1: backward-data    dst[tap'][co][ci]       = w[co][ci][dy][dx], tap' = (kh-1-dy)*kw + (kw-1-dx)
 *                  (the packed "cin" axis is then the forward cout and vice versa)
 * cin_keep: for transpose=1, only the first cin_keep forward input channels are produced (drops ctx grads).
 * Rows/cols beyond the real sizes are zero filled. */
int sda_pack_conv_weight(const float* w, int cout, int cin, int kh, int kw, int transpose, int cin_keep,
                         float* dst, int k_pad, int m_pad, void* stream);

/* Winograd-domain weights (G g G^T)[xi][nu] of 3 x 3 filters for sda_conv_desc.w_wino4 (transpose / cin_keep as above): dst[k_pad/8][16][m_pad/16][64][2], k_pad % 8 == 0, m_pad % 32 == 0 (ABI v13; % 96 before:
 * the layout is per 16-cout fragment and does not depend on the cout tile the kernel then picks from m_pad). */
int sda_pack_conv_weight_wino4(const float* w, int cout, int cin, int transpose, int cin_keep, float* dst, int k_pad,
                               int m_pad, void* stream);
/* The zero-position packing of a sda_pack_conv_weight_wino4 buffer (sda_conv_desc.w_wino4_zp): dst holds
 * sda_wino4_zp_floats(k_pad, m_pad) = (k_pad / 8) * (m_pad / T) * Z floats with (T, Z) = (96, 7168) for m_pad % 96 == 0, else (64, 5120)
 * for m_pad % 64 == 0, else (32, 3072) (ABI v13), [K stage][cout tile][Z]; for the 96-cout tile: the three position pairs
 * whose two positions are both live (6 x 256 float4 each), the live halves of the pairs (2, 3) and (6, 7) interleaved into one such block,
 * the live half of pair (14, 15) as 6 x 256 float2, zero padding to 28 KiB -- the order the kernel's LDS stage buffer has, so that a
 * helper wave copies seven linear 1-KiB pieces.  Values are copied, not recomputed: the kernels stay bit-identical to the full ones. */
int sda_pack_conv_weight_wino4_zp(const float* w_wino4, int k_pad, int m_pad, float* dst, void* stream);
int64_t sda_wino4_zp_floats(int k_pad, int m_pad);

/* ------------------------------------------------------------------------------------------
 * zuko.nn.LayerNorm(dim=-(spatial+1)) statistics: per pixel, over channels, of (x + mod).
 * Call sites sda/nn.py:137,163; algorithm zuko==0.1.4 (not in tree): mean, var (unbiased),
 * rstd = 1/sqrt(var+eps).  x planar [n][c][hw].  The normalisation itself is applied inside
 * the consuming conv's loader (sda_conv_igemm) or sda_ln_apply.
 * ------------------------------------------------------------------------------------------ */
int sda_ln_stats(const float* x, int n, int c, int hw, const float* mod, int64_t mod_sn, float eps, int unbiased,
                 float* mean, float* rstd, void* stream);
/* y = (x + mod - mean) * rstd   (materialised LN; used by tests and non-fused callers) */
int sda_ln_apply(const float* x, int n, int c, int hw, const float* mod, int64_t mod_sn, const float* mean,
                 const float* rstd, float* y, void* stream);
/* Backward of h = LN_c(x + mod) w.r.t. x (what autograd computes through sda/nn.py:137,163):
 *   gx = (res ? res : 0) + rstd * (gh - mean_c(gh) - h * sum_c(gh*h)/(c-1|c))
 * pool_h x pool_w: gh is given at that multiple of the resolution ([n][c][pool_h*h][pool_w*w]) and summed over each cell
 * first (backward of nn.Upsample nearest, sda/nn.py:164): 1x1 none, 2x2 for 2-D nets, 1x2 for 1-D nets (h == 1 there, but
 * h == 1 does not imply a 1-D net: the deepest level of a 2-D net may be one row high). */
int sda_ln_bwd(const float* gh, const float* x, int n, int c, int h, int w, const float* mod, int64_t mod_sn,
               const float* mean, const float* rstd, int unbiased, int pool_h, int pool_w, const float* res, float* gx,
               void* stream);
/* (ABI v12) the same, and amax[0] = max |gx| (device scalar, written by this call): the input scale of the OPT-IN f16 x 2 convolution
 * that reads gx next (sda_conv_desc.x_amax) without an sda_absmax pass -- reduced in the kernel's own epilogue on the U-Net levels'
 * 16-byte layouts, by an sda_absmax pass over gx otherwise. */
int sda_ln_bwd_amax(const float* gh, const float* x, int n, int c, int h, int w, const float* mod, int64_t mod_sn,
                    const float* mean, const float* rstd, int unbiased, int pool_h, int pool_w, const float* res, float* gx,
                    float* amax, void* stream);

/* ------------------------------------------------------------------------------------------
 * TimeEmbedding + every block's `project` Linear in one go (sda/score.py:15-35, sda/nn.py:132-135):
 *   feat = [cos(freqs*t), sin(freqs*t)]; emb = W2 silu(W0 feat + b0) + b2;  mod = Wp emb + bp
 * t: [nt] ; emb out: [nt][e]; mod out: [nt][cp]  (cp = sum of block widths, Wp = rows concatenated)
 * ------------------------------------------------------------------------------------------ */
int sda_time_embed(const float* t, int nt, const float* freqs, int nf, const float* w0, const float* b0, int hidden,
                   const float* w2, const float* b2, int e, float* emb, void* stream);
int sda_linear_small(const float* x, int rows, int in_f, const float* w, const float* b, int out_f, float* y,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * Fully-connected layers of ScoreNet / ResMLP (the Lorenz local kernel; sda/nn.py:31-71, sda/score.py:38-63), row-major
 * (rows, features) fp32, on the fp32 matrix cores:
 *   y = act_out( act_in(x) . Wop + b ) * act'(dact_z) + res
 *   trans_w = 0: Wop = w^T with w = torch's [out_f][in_f]  (forward of nn.Linear)
 *   trans_w = 1: Wop = w   with w = [in_f][out_f]          (backward-data of nn.Linear: gx = gy . W, pass in_f = W's out)
 * and zuko.nn.LayerNorm over the last axis (call site sda/nn.py:61) with its input gradient; one 64-lane wavefront per
 * row, shuffle reductions.
 * ------------------------------------------------------------------------------------------ */
int sda_linear(const float* x, int rows, int in_f, const float* w, const float* b, int out_f, int trans_w, int act_in,
               int act_out, const float* dact_z, int act_d, const float* res, float* y, void* stream);
int sda_row_ln(const float* x, int rows, int f, float eps, int unbiased, float* y, float* mean, float* rstd, void* stream);
int sda_row_ln_bwd(const float* gh, const float* x, int rows, int f, const float* mean, const float* rstd, int unbiased,
                   const float* res, float* gx, void* stream);

/* A whole ResMLP (sda/nn.py:31-71: per width step an optional Linear, then x + Lin2(act(Lin1(LN(x))))) in ONE launch, and its
 * input VJP in one more (csrc/mlp1d.hip; ABI v7) -- the Lorenz local score kernel of experiments/lorenz/utils.py:45-59.
 * The network is a list of GEMMs in forward order: kind 0 = nn.Linear; kind 1 = first half of a residual block (LayerNorm -> Linear ->
 * activation), always followed by kind 2 = its second half (Linear + residual).  Widths <= 256 (ABI v13; <= 128 before: a net whose
 * widths are all <= 128 runs the same kernels on the same bytes as then).
 *   w:    per GEMM one SLAB at float offset w_off[g] (a multiple of 4).  Both sides <= 128: the matrix Wp = W zero padded to
 *         [16 mf][16 kq] (mf = 1 if out <= 16 else 8 output fragments; kq = 1 / 4 / 8 K quads for in <= 16 / 64 / 128) in MFMA A-operand
 *         order [m mf][sq kq][lane 64][4] -- element e of lane (k = lane >> 4, li = lane & 15) = Wp[16 m + li][16 sq + 4 k + e] --, zero
 *         padded to a multiple of 4096 floats (one UNIT).  A side above 128 pads to 256 (mf = 16 / kq = 16) and splits in two halves of
 *         128: the slab is then the units of Wp's quarters Wp[128 nh ..][128 kh ..] (halves, when the other side is <= 128 -- that side
 *         keeps its own padding 16 / (64) / 128), each laid out and padded as above, in the order [output half nh][input half kh]:
 *         256 x 256 = 4 x 16384 floats, 47 -> 256 = 2 x 8192, 256 -> 15 = 2 x 4096.  sda_mlp_slab_floats(in, out) = the slab's length
 *         (SDA_E_UNSUPPORTED above 256).  sda_mlp_fwd: W = torch's [out][in] weight; sda_mlp_bwd: W = its transpose (the slab of
 *         (out -> in)), same offsets table;
 *   bias: [16 mf] zero padded at float offset b_off[g] (a multiple of 4; forward only).  All padded biases together: <= 4096 floats (they
 *         stay in LDS for the launch -- sixteen 256-wide GEMMs), else SDA_E_UNSUPPORTED;
 *   x / out: row-major (rows, features) with row strides x_ld / out_ld (sda_mlp_bwd: x = cotangent rows of width out_f[last], out =
 *         input-gradient rows of width in_f[0]).
 *   a_save / z_save [nres][rows][save_ld >= 128; >= 256 when a residual block is wider than 128], mean_save / rstd_save [nres][rows]
 *         (block strides save_stride / stat_stride): written by the forward when non-NULL (all four or none), read by the VJP.
 * SDA_E_UNSUPPORTED outside the kernel's range (callers run the per-layer kernels sda_linear / sda_row_ln). */
#define SDA_MLP_MAXG 32
typedef struct sda_mlp_desc {
    int32_t rows, ngemm;
    int32_t act, unbiased;
    float eps;
    int32_t kind[SDA_MLP_MAXG];
    int32_t in_f[SDA_MLP_MAXG], out_f[SDA_MLP_MAXG];
    int32_t w_off[SDA_MLP_MAXG], b_off[SDA_MLP_MAXG];
    const float* w; const float* bias;
    const float* x; int64_t x_ld;
    float* out; int64_t out_ld;
    float* a_save; float* z_save; int64_t save_stride; int32_t save_ld;
    float* mean_save; float* rstd_save; int64_t stat_stride;
} sda_mlp_desc;
int sda_mlp_fwd(const sda_mlp_desc* d, void* stream);
int sda_mlp_bwd(const sda_mlp_desc* d, void* stream);
int sda_mlp_slab_floats(int in_f, int out_f);         /* host, no launch */

/* Parameter gradients of the same chain (csrc/mlp_train.hip; opt-in training, sda_amd.training.parameter_gradients(mlp=True)).
 *
 * sda_mlp_bwd_train: sda_mlp_bwd on `mlp` (ONE kernel text, csrc/mlp1d_vjp_kernels.hpp, compiled into both entries: same transposed slabs,
 *   same saves, same input gradient bit for bit) that also stores the cotangent at every GEMM's OUTPUT as rows g_save[g][row][g_ld]
 *   (GEMM stride g_stride floats):
 *     kind 0: the cotangent of the Linear's output;  kind 2: the cotangent of the block's output;
 *     kind 1: gz = (g . W2) * act'(z), the cotangent of the pre-activation.
 *   Rows are written as whole 16-feature fragments: columns [out_f[g], padded width) of a row receive zeros, columns beyond the padded
 *   width (16 for out_f <= 16, else 128, else 256) are not touched.  g_ld >= the widest padded out_f, a multiple of 4; g_save 16-byte
 *   aligned, g_stride a multiple of 4.
 *
 * sda_mlp_wgrad: ONE launch for every GEMM of the chain, then one slab reduction:
 *     dw[g][o][i] (+)= sum_r G[r][o] U[r][i],   db[g][o] (+)= sum_r G[r][o]        (dw = torch's unpadded [out_f][in_f], db [out_f])
 *   on the fp32 matrix cores, G = g[g] (rows of g_save, row stride g_ld) and U rebuilt by the loader from what the forward saved:
 *     kind 0: src[g][r][i]                                   (the Linear's own input rows: the net input or a segment's output)
 *     kind 1: (src[g][r][i] - mean[g][r]) * rstd[g][r]       (src = the block's rows of a_save, mean / rstd its statistics)
 *     kind 2: act(src[g][r][i])                              (src = the block's rows of z_save)
 *   (row stride src_ld[g]).  The bias is one more column of the same multiply (U = 1).  The row axis is cut into `slabs` contiguous
 *   ranges (0 = the planner's choice, a function of the shapes only; 1 .. 64 = forced, clipped to the number of 32-row stages);
 *   unreduced partials go to work[sda_mlp_wgrad_work_floats(d)]; the second kernel sums them in slab order: no atomics, bitwise
 *   reproducible.  accumulate: add onto dw / db instead of overwriting.  db[g] may be NULL.  Nothing outside [out_f][in_f] / [out_f]
 *   is written.  SDA_E_UNSUPPORTED: rows < 1, ngemm outside 1 .. SDA_MLP_MAXG, a width outside 1 .. 256, a kind outside 0 .. 2;
 *   SDA_E_BADARG: null pointers, slabs outside 0 .. 64, row strides shorter than the width. */
typedef struct sda_mlp_train_desc {
    sda_mlp_desc mlp;
    float* g_save; int64_t g_stride; int32_t g_ld;
} sda_mlp_train_desc;
typedef struct sda_mlp_wgrad_desc {
    int32_t rows, ngemm;
    int32_t act;
    int32_t kind[SDA_MLP_MAXG];
    int32_t in_f[SDA_MLP_MAXG], out_f[SDA_MLP_MAXG];
    const float* src[SDA_MLP_MAXG]; int64_t src_ld[SDA_MLP_MAXG];
    const float* mean[SDA_MLP_MAXG]; const float* rstd[SDA_MLP_MAXG];
    const float* g[SDA_MLP_MAXG]; int64_t g_ld;
    float* dw[SDA_MLP_MAXG]; float* db[SDA_MLP_MAXG];
    float* work;
    int32_t slabs, accumulate;
} sda_mlp_wgrad_desc;
int sda_mlp_bwd_train(const sda_mlp_train_desc* d, void* stream);
int sda_mlp_wgrad(const sda_mlp_wgrad_desc* d, void* stream);
/* planning only (nothing is launched, `work` may be NULL): the slab count the launch will use / the floats of `work` it needs; <0 error */
int sda_mlp_wgrad_slabs(const sda_mlp_wgrad_desc* d);
int64_t sda_mlp_wgrad_work_floats(const sda_mlp_wgrad_desc* d);

/* The optimizer step of the same training route (csrc/optim.hip; sda_amd.training.AdamW): a multi-tensor AdamW with decoupled weight
 * decay over up to SDA_ADAMW_MAXT fp32 tensors in ONE launch, in the operation order of torch's single-tensor AdamW:
 *     p = p * decay;   m = m + (g - m) * one_m_beta1;   v = v * beta2 + (one_m_beta2 * g) * g;
 *     p = p - step_size * (m / (sqrt(v) * rsqrt_bc2 + eps))
 *   with decay = 1 - lr wd, step_size = lr / (1 - beta1^t), rsqrt_bc2 = 1 / sqrt(1 - beta2^t) formed by the caller in double and passed
 *   as fp32.  p, m, v [numel] are updated in place; g is read.
 * The pack epilogue keeps a sda_mlp_desc's slabs valid without a re-pack: a tensor with pack_kind 1 is a GEMM weight [out_f][in_f]
 *   (numel = out_f in_f, both sides 1 .. 256) whose new value p[o][i] also goes to fwd[pos(out_f, in_f, o, i)] and bwd[pos(in_f, out_f, i, o)]
 *   -- fwd / bwd = the GEMM's forward / transposed slab (w + w_off[g] of the two weight buffers), pos = the slab order described at
 *   sda_mlp_desc above --; pack_kind 2 is a bias [numel] whose new value also goes to fwd[o] (bias + b_off[g]).  The zero padding of the
 *   slabs is never written.
 * Block b of the launch updates chunk b - blk0[t] (1024 elements) of the tensor t with blk0[t] <= b < blk0[t + 1]; sda_adamw_step fills
 *   blk0 itself (callers leave it alone).  Every output element has one writer and there are no atomics: bitwise reproducible.
 * SDA_E_BADARG: a null descriptor or p / g / m / v, ntensor outside 1 .. SDA_ADAMW_MAXT, numel < 1, a pack_kind outside 0 .. 2, a weight
 *   whose numel is not out_f in_f, a null fwd (kinds 1, 2) or bwd (kind 1); SDA_E_UNSUPPORTED: a weight side outside 1 .. 256, more than
 *   2^31 - 1 blocks.  Nothing is launched then. */
#define SDA_ADAMW_MAXT 32
typedef struct sda_adamw_desc {
    int32_t ntensor;
    float decay, one_m_beta1, beta2, one_m_beta2, step_size, rsqrt_bc2, eps;
    float* p[SDA_ADAMW_MAXT]; const float* g[SDA_ADAMW_MAXT];
    float* m[SDA_ADAMW_MAXT]; float* v[SDA_ADAMW_MAXT];
    float* fwd[SDA_ADAMW_MAXT]; float* bwd[SDA_ADAMW_MAXT];
    int64_t numel[SDA_ADAMW_MAXT];
    int32_t pack_kind[SDA_ADAMW_MAXT];                 /* 0 none, 1 GEMM weight, 2 bias */
    int32_t out_f[SDA_ADAMW_MAXT], in_f[SDA_ADAMW_MAXT];
    int32_t blk0[SDA_ADAMW_MAXT + 1];                  /* filled by sda_adamw_step */
} sda_adamw_desc;
int sda_adamw_step(const sda_adamw_desc* d, void* stream);
/* The same launch for a replayed (hipGraph) training step (additive, ABI stays v14): row table[irow[0]] = {decay, step_size, rsqrt_bc2} of a
 *   device table replaces the descriptor's three by-value fields of those names (which are not read); everything else -- the checks, blk0,
 *   the per-thread update, the pack epilogue -- is sda_adamw_step's.  irow: a device int64 scalar the caller keeps inside the table and
 *   advances on the device after the step's last launch.  SDA_E_BADARG also for a null table or irow. */
int sda_adamw_step_dev(const sda_adamw_desc* d, const float* table, const int64_t* irow, void* stream);

/* The denoising loss of the training route as replayable launches (csrc/train_loss.hip; additive, ABI stays v14): what
 * `t = torch.rand(B); eps = randn_like(x); xt = mu(t) x + sigma(t) eps; ((net(xt, t) - eps)**2).mean()` (sda/score.py:195-223, 265-276)
 * makes of some fifteen torch launches and two draws of torch's generator.
 * sda_loss_perturb: x [rows][per_row] -> t [rows], eps and xt [rows][per_row] in one launch.  eps[b] is BY DEFINITION row row0 + b of
 *   sda_randn_rows(seed, draw = 2 s); t[b] = ((w0 >> 8) + 0.5) 2^-24 in (0, 1), w0 = word 0 of the same generator at quad 0 of row row0 + b in
 *   draw 2 s + 1.  s = step_dev[0] (a device int64 scalar: the launch is hipGraph-replayable) or, with step_dev NULL, `step`.  mu(t[b]) and
 *   sigma(t[b]) are sda_vp_schedule's (same device function, same alpha_kind / eta / k / sigma_kind); xt = mu x + sigma eps, two products and
 *   a sum, each rounded on its own.  SDA_E_BADARG: a null pointer, rows < 1, per_row < 1, row0 < 0, step < 0, an unknown kind;
 *   SDA_E_UNSUPPORTED: more than 2^31 - 1 workgroups (rows * ceil(per_row / 1024)).
 * sda_loss_mse: loss[0] = mean((out - eps)^2) over numel contiguous elements and, with g != NULL, g = (2 / numel) (out - eps) -- the
 *   loss's cotangent at out for an upstream gradient of 1 (difference, fp32 scale 2 / numel, product: three roundings).  Two ordered stages
 *   (per-workgroup partial sums into `work`, then one workgroup in index order), no float atomics: bitwise reproducible.  `work` holds
 *   sda_loss_mse_plan(numel, ...) floats.
 * sda_loss_mse_plan: floats of `work` = workgroups of stage 1 (*blocks; chunks of 4096 elements), and *chain = the longest chain of
 *   additions any term passes through: 16 in its thread, 6 + 3 in its workgroup's tree, ceil(blocks / 256) in stage 2's thread, 6 + 3 in
 *   stage 2's tree.  Either pointer may be NULL.  < 0: SDA_E_BADARG (numel < 1) / SDA_E_UNSUPPORTED (more than 2^31 - 1 workgroups). */
int sda_loss_perturb(const float* x, int rows, int64_t per_row, uint64_t seed, int64_t row0, int64_t step, const int64_t* step_dev,
                     int alpha_kind, float eta, float k, int sigma_kind, float* t, float* eps, float* xt, void* stream);
int64_t sda_loss_mse_plan(int64_t numel, int* blocks, int* chain);
int sda_loss_mse(const float* out, const float* eps, int64_t numel, float* loss, float* g, float* work, void* stream);

/* The device-resident trajectory dataset (csrc/dataset.hip; additive, ABI stays v14): what a shuffled DataLoader over the reference's
 * TrajectoryDataset (sda/utils.py:58-86: one randint, one narrow, one flatten per item, then collation and an upload) feeds a training
 * step, as one launch.  data [N][L][F] contiguous fp32 (N trajectories, L frames, F values per frame) -> out [rows][W F]: row b holds the
 * W F contiguous values from ((n_b L) + start_b) F on.
 * sda_window_batch: the global batch index is s = step_dev[0] (a device int64 scalar the launch only reads: hipGraph-replayable) or, with
 *   step_dev NULL, `step`.  spe = ceil(N / batch); epoch e = s / spe, batch i = s % spe, position p = i batch + b.  n_b = perm_e(p), a
 *   permutation of [0, N) keyed on (seed, e): a four-round balanced Feistel network over 2h-bit words (4^h the smallest power of four
 *   >= N) with cycle walking, round function = word 0 of Philox4x32-10 at counter {v, e_lo, 0x80000000 | e_hi, 'SHU0' + round};
 *   start_b = (u (L - W + 1)) >> 32 (64-bit product), u = word 0 at counter {b, s_lo, 0x80000000 | s_hi, 'WSTA'}; key = seed in both.
 *   Neither counter collides with sda_randn_rows' or sda_bpf_resample's (csrc/philox.hpp): the seed of the loss noise may be reused.
 *   The caller passes the rows of this batch by value (rows <= batch; the epoch's short last batch is a launch with fewer rows) and
 *   guarantees i batch + rows <= N; with a device counter, rows past the epoch's end are left unwritten.  16-byte copies where
 *   F % 4 == 0 and data / out are 16-byte aligned, scalar ones otherwise.
 * sda_window_batch_plan: host only -- the same (n_b, start_b), from the same index functions, for `rows` rows of batch `step` into two
 *   int64 host arrays.
 * Both: SDA_E_BADARG for a null pointer, N, L, F, W, batch or rows < 1, W > L, rows > batch, step < 0, or a by-value step with
 *   i batch + rows > N (sda_window_batch ignores the by-value step's position when step_dev is given); SDA_E_UNSUPPORTED for N, L or
 *   batch >= 2^31, more than 2^31 - 1 workgroups (rows * ceil(W F / 1024)) or N L F past an int64 offset. */
int sda_window_batch(const float* data, int64_t N, int64_t L, int64_t F, int64_t W, int64_t batch, int64_t rows, uint64_t seed,
                     int64_t step, const int64_t* step_dev, float* out, void* stream);
int sda_window_batch_plan(int64_t N, int64_t L, int64_t W, int64_t batch, uint64_t seed, int64_t step, int64_t rows, int64_t* src_row,
                          int64_t* start);

/* The same two launches as the halves of a Gaussian-guided evaluation of a LOCAL score network -- MCScoreNet over a ScoreNet kernel
 * (sda/score.py:134-164, 53-63; experiments/lorenz/utils.py:45-59) inside GaussianScore (score.py:375-396) --, the rows being the
 * nw = len - 2k windows of each of rows / nw trajectories x (B, len, c), wc = (2k + 1) c <= 32 (a window's values fill one or two 16-feature
 * fragments of the kernels; above 32 sda_mlp_fwd_win / sda_mlp_bwd_win return SDA_E_UNSUPPORTED and sda_mc_finish SDA_E_BADARG):
 *   sda_mlp_fwd_win: the loader gathers a window's (2k + 1) c consecutive values and appends the time embedding emb[emb_n]
 *                    (`unfold`, `cat`: in_f[0] = (2k + 1) c + emb_n); the epilogue applies `fold` (score.py:155-164), forms
 *                    eps = (cx0 + cx1 sigma) x + cn s and the likelihood cotangent ghat exactly as sda_net1d_fwd_fused does, and writes both
 *                    as (B, len, c) tensors (d.x / d.out are unused);
 *   sda_mlp_bwd_win: the loader applies fold's adjoint to cn ghat; the window part of the input gradient leaves as gwin [rows][16] when
 *                    wc <= 16 and as gwin [rows][32] when 16 < wc <= 32 (16-byte aligned; value f of a row at offset f, the rest of the
 *                    row up to the last whole fragment is written too).  Both sides derive the row stride from nw, len / k and c:
 *                    there is no stride argument;
 *   sda_mc_finish:   reads gwin with that stride (wc <= 16 ? 16 : 32), sums the overlapping windows (unfold's adjoint, in ascending slot
 *                    order), adds the affine part, forms the guided score
 *                    eps - (sigma/mu)(ghat - sigma J_eps^T ghat) and, by mode (as sda_net1d_bwd_fused): 0 writes it; 1 x <- r x + c1 . in
 *                    place; 2 writes it and partial[b] = its sum of squares over the trajectory (one chunk per sample).
 * A last GEMM of 17 .. 32 outputs (and its transpose, the VJP's first) is a 128-feature slab like any width above 16: at wc = 21 or 27 these
 * two multiplies do 128-wide work for 21 or 27 useful columns. */
typedef struct sda_mlp_win {
    int32_t nw, len, c, emb_n;
    const float* x; const float* emb;
    float cx0, cx1, cn;
    const float* coef;                 /* device {mu(t), sigma(t)} */
    const float* y; int64_t y_sn;
    int32_t p_start, p_step, p_stop, c_start, c_step, c_stop;
    float std, gamma;
    float* eps; float* ghat;           /* fwd: out; bwd: ghat in */
    float* gwin;                       /* bwd: out */
} sda_mlp_win;
int sda_mlp_fwd_win(const sda_mlp_desc* d, const sda_mlp_win* w, void* stream);
int sda_mlp_bwd_win(const sda_mlp_desc* d, const sda_mlp_win* w, void* stream);
int sda_mc_finish(const float* eps, const float* ghat, const float* gwin, int b, int nw, int k, int c, float cx0, float cx1,
                  const float* coef, int mode, float* out, float* xs, const float* step_coef, float* partial, void* stream);

/* ------------------------------------------------------------------------------------------
 * MCScoreNet.fold (sda/score.py:155-164): selective gather, NOT an overlap-add.
 *   s: [b][nw][(2k+1)*c][hw] -> out: [b][nw+2k][c][hw]
 * and the adjoints needed for the guidance gradient (sda/score.py:394):
 *   fold_adjoint:   g_out [b][l][c][hw] -> g_s [b][nw][(2k+1)c][hw]  (zero where fold does not read)
 *   unfold_adjoint: g_win [b][nw][(2k+1)c][hw] -> g_x [b][l][c][hw] (+= overlapping windows; the one place overlaps sum)
 * ------------------------------------------------------------------------------------------ */
int sda_fold(const float* s, int b, int nw, int k, int c, int hw, float* out, void* stream);
int sda_fold_adjoint(const float* g_out, int b, int nw, int k, int c, int hw, float* g_s, void* stream);
int sda_unfold_adjoint(const float* g_win, int b, int nw, int k, int c, int hw, int64_t win_sc_total, float* g_x,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * Predictor-corrector updates of VPSDE.sample (sda/score.py:250-261).
 *   predict:  x = r*x + c1*eps                                                (score.py:252-253)
 *   sumsq:    partial[b][j] = sum over chunk j of eps[b]^2  (deterministic two-stage mean, score.py:259)
 *   correct:  delta = tau / mean(eps^2); x = x - (delta*eps + sqrt(2 delta)*z)*sigma   (score.py:259-261)
 * coef: device pointer to {r, c1} / {sigma} when coef_dev != NULL (graph replay), else the by-value scalars.
 * ------------------------------------------------------------------------------------------ */
/* out2 = {mu(t), sigma(t)} of the VP / sub-VP / sub-sub-VP schedules (sda/score.py:195-210, 279-302) for a device scalar t.
 * alpha_kind 0 'lin', 1 'cos' (k = acos(sqrt(eta))), 2 'exp' (k = log(eta)); sigma_kind 0 VPSDE, 1 SubVPSDE, 2 SubSubVPSDE. */
int sda_vp_schedule(const float* t, int alpha_kind, float eta, float k, int sigma_kind, float* out2, void* stream);
int sda_pc_predict(float* x, const float* eps, int64_t numel, float r, float c1, const float* coef_dev, void* stream);
int sda_sumsq_partial(const float* eps, int b, int64_t per_sample, float* partial, int nchunk, void* stream);
int sda_pc_correct(float* x, const float* eps, const float* z, int b, int64_t per_sample, const float* partial,
                   int nchunk, float tau, float sigma, const float* coef_dev, void* stream);

/* Corrector noise z ~ N(0, I) (the torch.randn_like(x) of sda/score.py:257) keyed per ROW, for batch-sharded runs:
 *   out[r][j], r in [0, rows), depends on (seed, row0 + r, draw, j) only -- Philox4x32-10 with counter
 *   {j/4, row, draw} and key = seed, Box-Muller on 24-bit uniforms -- so every world size draws the same noise for the
 *   same trajectory and each rank generates its own rows only.  draw_dev (optional): the draw index is
 *   draw_dev[0] * draw_mul + draw_add, read on the device (a step counter) => the launch is hipGraph-replayable.
 * sda_philox_words: the raw generator words for counter {i, c1, c2, c3}, i in [0, n) (4 uint32 each; tests). */
int sda_randn_rows(float* out, int rows, int64_t per_row, uint64_t seed, int64_t row0, int64_t draw,
                   const int64_t* draw_dev, int64_t draw_mul, int64_t draw_add, void* stream);
int sda_philox_words(uint32_t* out, int64_t n, uint64_t seed, uint32_t c1, uint32_t c2, uint32_t c3, void* stream);

/* Gaussian-guidance elementwise pieces (sda/score.py:387,396):
 *   xhat = (x - sigma*eps)/mu ;   out = eps - (sigma/mu)*(ghat - sigma*vjp),  vjp = J_eps^T ghat
 * coef_dev (optional): device {mu, sigma} overriding the by-value scalars (no host sync, graph replay). */
int sda_denoise(const float* x, const float* eps, int64_t numel, float mu, float sigma, const float* coef_dev,
                float* xhat, void* stream);
int sda_guided_combine(const float* eps, const float* ghat, const float* vjp, int64_t numel, float mu, float sigma,
                       const float* coef_dev, float* out, void* stream);
/* out = (y - ax) / (std^2 + gamma (sigma/mu)^2): the cotangent of log N(y | A x_hat, var) (sda/score.py:389-392) for scalar
 * std / gamma; y broadcasts over the leading axis (y_numel divides numel); (mu, sigma) from coef_dev when non-NULL */
int sda_gauss_cotangent(const float* y, int64_t y_numel, const float* ax, int64_t numel, float std, float gamma, float mu,
                        float sigma, const float* coef_dev, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Linear observation operators A of the reference's experiments and their adjoints A^T, so that GaussianScore
 * (sda/score.py:387-394) needs no autograd through A: d log p / d x_hat = A^T((y - A x_hat)/var).
 *   subsample: a 5-D strided slice x[..., start::step, ...] (experiments/lorenz/eval.py:75; kolmogorov/figures.ipynb#cell30-39)
 *   coarsen:   KolmogorovFlow.coarsen, block mean over f x f cells      (sda/mcs.py:340-347)
 *   vorticity: KolmogorovFlow.vorticity, periodic central differences   (sda/mcs.py:361-375); x = [pairs][2][h][w]
 * size5/start5/step5: host int[5] (leading dims padded with size 1, start 0, step 1).
 * ------------------------------------------------------------------------------------------ */
int sda_obs_subsample(const float* x, const int* size5, const int* start5, const int* step5,
                      const int* stop5 /* exclusive ends per dim (a crop, figures.ipynb#cell16,23), or NULL */, float* out, void* stream);
int sda_obs_subsample_adjoint(const float* r, const int* size5, const int* start5, const int* step5, const int* stop5, float* gx,
                              void* stream);
/* g = A^T((y - A((x - sigma eps)/mu)) / (std^2 + gamma (sigma/mu)^2)) for the subsampling A above, scalar std / gamma, in one
 * launch (sda/score.py:387-394); y broadcasts over the leading axis; (mu, sigma) from coef_dev when non-NULL */
int sda_obs_subsample_guidance(const float* x, const float* eps, const float* y, int64_t y_numel, const int* size5,
                               const int* start5, const int* step5, const int* stop5 /* exclusive ends per dim, or NULL */,
                               float std, float gamma, float mu, float sigma, const float* coef_dev, float* g, void* stream);
int sda_obs_coarsen(const float* x, int64_t planes, int h, int w, int f, float* out, void* stream);
int sda_obs_coarsen_adjoint(const float* r, int64_t planes, int h, int w, int f, float* gx, void* stream);
int sda_obs_vorticity(const float* x, int64_t pairs, int h, int w, float* out, void* stream);
int sda_obs_vorticity_adjoint(const float* r, int64_t pairs, int h, int w, float* gx, void* stream);
/* The non-linear / masked / coupled observations of the reference's experiments with the VJP of their
 * linearisation, so that the guidance gradient d log p / d x_hat = J_A(x_hat)^T((y - A x_hat)/var) (sda/score.py:389-394)
 * needs no autograd through A:
 *   pointwise kind 1: w / (1 + |w|)  (the saturating sensor of kolmogorov/figures.ipynb#cell23), 2: tanh, 3: w^2, 4: |w|;
 *             _vjp: gx = r * f'(x)
 *   mask:     out = x * m, m broadcast over the leading dims (m_numel divides n)   (figures.ipynb#cell4); self-adjoint
 *   timediff: x [outer][len][inner] -> x[:, i] - x[:, j]  (the loop closure x[:, 0] - x[:, -1] of figures.ipynb#cell43);
 *             _adjoint: gx = +r at index i, -r at index j, 0 elsewhere */
int sda_obs_pointwise(const float* x, int64_t n, int kind, float* out, void* stream);
int sda_obs_pointwise_vjp(const float* x, const float* r, int64_t n, int kind, float* gx, void* stream);
int sda_obs_mask(const float* x, int64_t n, const float* m, int64_t m_numel, float* out, void* stream);
int sda_obs_timediff(const float* x, int64_t outer, int len, int64_t inner, int i, int j, float* out, void* stream);
int sda_obs_timediff_adjoint(const float* r, int64_t outer, int len, int64_t inner, int i, int j, float* gx, void* stream);

/* ------------------------------------------------------------------------------------------
 * Evaluation metrics of the sampling experiments.
 *   sda_pairwise_dist   : out[i][j] = |x_i - y_j|^2 (take_sqrt = 0) or |x_i - y_j| (1); x [m][d], y [n][d], out [m][n].
 *                         Replaces torch.cdist in emd (sda/utils.py:215-219) and the Gram-matrix expansion of mmd
 *                         (sda/utils.py:236-250).
 *   sda_mmd_kernel_sums : partial[b] = sum over a grid-stride slice of d2[0..count) of
 *                         sum_{sigma in 1e-3..1e3} exp(-d2/sigma)   (sda/utils.py:252-261); partial: nblocks doubles.
 *   sda_assignment_cost : HOST pointers.  min over permutations of sum_i cost[i][p(i)] -- the optimal transport LP of
 *                         ot.emd2 (sda/utils.py:215) for uniform weights and equally many samples (POT, a third-party CPU
 *                         solver, is not vendored by the reference); col_of_row (optional) receives the permutation.
 * ------------------------------------------------------------------------------------------ */
int sda_pairwise_dist(const float* x, int m, const float* y, int n, int64_t d, int take_sqrt, float* out, void* stream);
int sda_mmd_kernel_sums(const float* d2, int64_t count, double* partial, int nblocks, void* stream);
int sda_assignment_cost(const float* cost, int n, double* total, int* col_of_row);
/*   sda_transport_cost : HOST pointers.  The same LP for m != n samples (uniform marginals 1/m, 1/n; sda/utils.py:203-219 with
 *       unequal sample counts): *total = min_P <P, cost>, an integral min-cost flow after scaling by m n.  cost: m x n row-major,
 *       finite and >= 0. */
int sda_transport_cost(const float* cost, int m, int n, double* total);
/*   sda_assignment_auction : DEVICE pointers.  The assignment problem of sda_assignment_cost -- the arithmetic of ot.emd2 in
 *       sda/utils.py:203-219 for uniform weights and equally many samples -- solved where the cost matrix already is: a forward
 *       auction with epsilon-scaling, one workgroup per problem, `batch` problems per launch (cost: [batch][n][n] fp32 row-major,
 *       4-byte aligned; 16-byte loads when n % 4 == 0 and the matrix is 16-byte aligned).  Phases run eps = R / 4, / 4, ... down
 *       to eps_final = eps_rel R, R = max cost - min cost; prices and bids are float64.  Per problem b:
 *         col_of_row[b][n]  the permutation (-1 for a row left unassigned when not converged)
 *         total[b]          sum_i cost[i][col_of_row[i]]                                    (float64, fixed summation order)
 *         gap[b]            total - (sum_i min_j (cost_ij + p_j) - sum_j p_j) >= total - optimum: a certificate that holds for any
 *                           prices p; the auction guarantees gap <= n eps_final
 *         eps_final[b], bids[b] (row scans done; <= bid_budget)
 *         status[b]         SDA_AUCTION_CONVERGED, SDA_AUCTION_NOT_CONVERGED (bid_budget would have been exceeded: total and gap are
 *                           NaN) or SDA_E_BADARG (a NaN / inf cost, as sda_assignment_cost answers; nothing else is meaningful)
 *       Results do not depend on scheduling: ties go to the lowest column (rows) and the lowest row (columns).
 *       Returns SDA_E_UNSUPPORTED for n > SDA_AUCTION_MAX_N (the state lives in LDS; nothing is launched), SDA_E_BADARG for null
 *       pointers, n, batch or bid_budget < 1, eps_rel outside [1e-12, 1]. */
#define SDA_AUCTION_MAX_N 4096
#define SDA_AUCTION_CONVERGED 0
#define SDA_AUCTION_NOT_CONVERGED 1
int sda_assignment_auction(const float* cost, int n, int batch, double eps_rel, int64_t bid_budget, double* total, double* gap,
                           double* eps_final, int64_t* bids, int32_t* status, int32_t* col_of_row, void* stream);

/* ------------------------------------------------------------------------------------------
 * 3-D convolutions: `UNet(spatial=3)` (sda/nn.py:114-118 picks nn.Conv3d; heads / residual blocks / tails as nn.py:148-206).
 * One gather kernel (implicit GEMM on v_mfma_f32_16x16x4_f32, B operand read from the planar tensor) for every launch of the
 * forward pass and of the input VJP.  Per axis a (d, h, w order):  v = o * stride[a] + tap - pad[a];  circular: v mod V,
 * zeros: taps outside [0, V) contribute nothing;  up[a] > 1: source = v / up[a]  (nn.Upsample(nearest) in the loader,
 * nn.py:164);  dil[a] > 1: source = v / dil[a] iff dil[a] divides v  (zero insertion: the transposed stride-2 convolution,
 * backward of nn.py:152-159).  V = in * up (or, zero-inserted: in * dil circular / (in - 1) * dil + 1 zeros).
 * Loader: act_in(x) on the gathered values (padding stays zero).
 * Epilogue: + bias[cout]; then x act'(z) if z else act(.); then + res.   x: [n][cin][in_size d,h,w], out / z / res:
 * [n][cout][out_size d,h,w], all contiguous.  w: sda_pack_conv3d_weight's layout (transpose = 1: the VJP operator --
 * taps flipped, cin <-> cout; `cin` / `cout` of the descriptor are then the operator's own).
 *   sda_pool3d_sum: adjoint of nearest up-sampling -- out[nc][d][h][w] = sum over the fd x fh x fw cell of g.
 * ------------------------------------------------------------------------------------------ */
typedef struct sda_conv3d_desc {
    const float* x;
    const float* w;
    const float* bias;      /* NULL: none */
    const float* z;         /* NULL: apply act; else multiply by act'(z) */
    const float* res;       /* NULL: none */
    float* out;
    int32_t n, cin, cout;
    int32_t in_size[3], out_size[3];
    int32_t k[3], pad[3], stride[3], up[3], dil[3];
    int32_t circular, act;
    int32_t act_in;         /* activation applied to x by the loader (the conv behind the block's activation, nn.py:139) */
} sda_conv3d_desc;
int sda_conv3d(const sda_conv3d_desc* d, void* stream);
int64_t sda_conv3d_packed_floats(int cout, int cin, int kd, int kh, int kw, int transpose);
int sda_pack_conv3d_weight(const float* w, int cout, int cin, int kd, int kh, int kw, int transpose, float* dst, void* stream);
int sda_pool3d_sum(const float* g, int64_t nc, int d, int h, int w, int fd, int fh, int fw, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Measurement support (ABI v10; no counterpart in the reference, which has no measurement code -- SURVEY.md section 6):
 * the shader clock the fp32 matrix-core stream sustains on this device.  `blocks` workgroups of 256 threads each issue
 * iters x 8 v_mfma_f32_16x16x4_f32 per wave from registers; out[2 b] = shader cycles (s_memtime), out[2 b + 1] = 100 MHz ticks
 * (s_memrealtime) workgroup b's first wave saw across its stream: clock = cycles / ticks x 100 MHz.  `sink`: one float of scratch.
 * bench.py runs it after the warm-up steps and reports roofline.frac next to the clock it was measured at.
 * ------------------------------------------------------------------------------------------ */
int sda_clock_probe(unsigned long long* out, int blocks, float* sink, int iters, void* stream);

/* ------------------------------------------------------------------------------------------
 * OPT-IN f16 x 2 emulation of the fp32 multiply (ABI v11; csrc/conv_h2.hip; see sda_conv_desc.w_h2).  Same layers as the
 * w_wino4 kernel -- the block convolutions nn.Conv2d(3 x 3) of sda/nn.py:131-142 and their backward-data -- as a DIRECT
 * convolution on v_mfma_f32_16x16x32_f16: x w ~ hi_x hi_w + hi_x lo_w + lo_x hi_w, fp32 accumulation.
 *   sda_conv_h2: the launch (SDA_E_UNSUPPORTED outside the range above: run sda_conv_igemm); sda_conv_h2_supported: 1 / 0, no launch.
 *   sda_pack_conv_weight_h2: torch-layout [cout][cin][3][3] -> fragments in MFMA lane order (transpose = 1: the input-VJP operator,
 *     taps flipped, cin <-> cout), w_amax = max |w| (host); sda_conv_h2_packed_bytes: size of dst (0: shape not served).
 *   sda_conv_h2_scale: the power of two s with s amax in [2^10, 2^11].   sda_absmax: amax[0] = max |x| (device scalar).
 * ------------------------------------------------------------------------------------------ */
int sda_conv_h2(const sda_conv_desc* d, void* stream);
int sda_conv_h2_supported(const sda_conv_desc* d);
int sda_pack_conv_weight_h2(const float* w, int cout, int cin, int transpose, float w_amax, void* dst, void* stream);
int64_t sda_conv_h2_packed_bytes(int cout, int cin, int transpose);
/* (ABI v12) the f16 x 2 form of a 3 x 3 convolution over a 2 x 2 nearest-up-sampled source (sda_conv_desc.up_h = up_w = 2: the tails,
 * sda/nn.py:161-169).  Output pixel (2 i + py, 2 j + px) sees only the 2 x 2 source pixels (i - 1 + py + a, j - 1 + px + b): each output
 * parity class is a 2 x 2-tap convolution of the low-resolution image with the taps that fall on one source pixel summed -- 4 / 9 of the
 * multiplies.  wsum: [4 classes (2 py + px)][cout][cin][4 taps (2 a + b)], summed in fp32 by the caller (class 0 rows: dy {0} | {1, 2};
 * class 1 rows: {0, 1} | {2}; columns alike), w_amax = max |wsum|.  A descriptor with up_h = up_w = 2 takes w_h2 = this packing;
 * served for cin % 32 == 0, cout a multiple of 96 or of 64 (ABI v13), a 16 x 16-tileable SOURCE grid, loader none / (modulation +) LayerNorm, epilogues bias / + res. */
int sda_pack_conv_weight_h2_up(const float* wsum, int cout, int cin, float w_amax, void* dst, void* stream);
int64_t sda_conv_h2_up_packed_bytes(int cout, int cin);
/* (ABI v12) generic form of the packing: w [rows][k][ntap] (ntap 1, 2, 4 or 9; rows a multiple of 96 or of 64 -- the cout tile the kernel runs --, k % 32 == 0: ABI v13).  The VJP of an up-sampled tail
 * summed over the 2 x 2 up-sampling cells (sda_conv_desc.pool_h = pool_w = 2) runs as a 2 x 2-tap convolution over the four parity planes
 * of the fine-resolution gradient: rows = the forward cin, k = 4 classes x the forward cout (class-major), ntap = 4,
 * w[ci][class * cout + co][tap] = wsum[class][co][ci][tap] of sda_pack_conv_weight_h2_up.  Served for a 32 x 32-tileable source, plain loader,
 * no bias / epilogue operand. */
int sda_pack_conv_weight_h2_rows(const float* w, int rows, int k, int ntap, float w_amax, void* dst, void* stream);
int64_t sda_conv_h2_rows_packed_bytes(int rows, int k, int ntap);
float sda_conv_h2_scale(float amax);
int sda_absmax(const float* x, int64_t numel, float* amax, void* stream);

/* ------------------------------------------------------------------------------------------
 * Markov chains and the bootstrap particle filter (csrc/chain.hip; additive, ABI stays v13): the simulators of sda/mcs.py:85-241
 * (DiscreteODE.transition = `steps` RK4 sub-steps of dt / steps, k1..k4 in the reference's operation order, fp32) and the filter
 * of sda/utils.py:168-200 as one launch per PHASE -- advance (+ log-weights), cdf, resample, and one traceback at the end.  No
 * kernel waits for another workgroup.
 *
 * sda_chain_advance: m particle states [m][d] (particle stride in_sp floats, components contiguous), optionally read through an
 *   ancestor vector (x_in[anc[j]]), advanced `transitions` >= 1 times in ONE launch.  every = 0: out[j * out_sp + c] = the last
 *   state; every = 1: out[t * out_st + j * out_sp + c] = the state after transition t (so a caller gets (length, m, d) or
 *   (m, length, d) by its choice of strides).  model.noise_std > 0 adds noise_std * z after every transition, where the z of particle
 *   slot j at transition t is BY DEFINITION row j of sda_randn_rows(out[m][d], seed, row0, draw = draw0 + t): same counters, same
 *   Box-Muller, so it does not depend on the launch geometry.  obs != NULL (kinds 0 and 1 only): the log-weights of
 *   sda_bpf_logweights for the LAST state, in the same launch.
 *   Lorenz-63 / Lotka-Volterra: one particle per lane, state in registers.  Lorenz-96 (4 <= d <= 64): a particle's components on the
 *   lanes of a sub-group of a wave (width = next power of two >= d), the rolls are cross-lane shuffles with the index modulo d.
 * sda_chain_log_prob: out[b] = sum_i sum_c log N(x[b][i+1][c]; RK4(x[b][i])[c], model.noise_std) (NoisyLorenz63.log_prob summed over
 *   the trajectory, experiments/lorenz/utils.py:82-88); x strides sb (trajectory) / sl (time) floats; the sum is float64.
 * sda_bpf_logweights: logw[j] = sum_k log N(y[k]; (x[j][idx[k]] - shift[k]) / scale[k], sigma) and pmax[workgroup] = the maximum over
 *   the workgroup's 256 particles (sda_bpf_logweights_blocks(m) values).
 * sda_bpf_cdf: w[j] = expf(logw[j] - max logw) (fp32) and cdf[j] = w[0] + ... + w[j] in float64, un-normalised; any m >= 1 (one
 *   workgroup walks the vector in chunks).  pmax may be NULL (the maximum is then taken over logw).  status[0] = 0, or 1 when every
 *   logw is -inf or any is NaN (cdf is then the uniform j + 1, so that a later resample stays defined); read it once, at the end.
 * sda_bpf_resample: anc[j] = the smallest i with cdf[i] > u cdf[m - 1], clamped to m - 1 (binary search), u in (0, 1) = (2 v + 1) / 2^53
 *   with v = the 52 bits (w0 >> 6) * 2^26 + (w1 >> 6) of the Philox counter {j_lo, obs_lo, 0x80000000 | j_hi, 'RESA'} under the
 *   key `seed`: i.i.d. categorical draws with replacement (torch.multinomial(w, m, replacement=True)).  Noise counters have bit
 *   31 of word 2 clear for t < 2^31 (csrc/philox.hpp), so the two streams never meet.
 * sda_bpf_traceback: S[t][slot][d] (strides s_st / s_sp) = the UN-resampled states t = 0 .. n_obs * step, anc[k][m] = the ancestors drawn
 *   at observation k; out[j][t][d] (contiguous) = the trajectory the reference obtains by re-gathering the whole history at every
 *   observation: i_N = j, i_k = anc[k][i_{k+1}], times k step + 1 .. (k + 1) step from S[t][i_k], time 0 from S[0][i_0].
 * ------------------------------------------------------------------------------------------ */
#define SDA_CHAIN_LORENZ63 0        /* p = {sigma, rho, beta}          d = 3 */
#define SDA_CHAIN_LOTKA_VOLTERRA 1  /* p = {alpha, beta, delta, gamma} d = 2 */
#define SDA_CHAIN_LORENZ96 2        /* p = {F}                         4 <= d <= 64 */
#define SDA_CHAIN_MAXOBS 64
typedef struct {
    int32_t kind, d, steps;
    float h;                /* dt / steps, rounded to fp32 */
    float p[4];
    float noise_std;        /* 0: deterministic */
} sda_chain_model;
typedef struct {
    int32_t k;              /* observed components, 1 <= k <= d */
    int32_t idx[SDA_CHAIN_MAXOBS];
    float shift[SDA_CHAIN_MAXOBS], scale[SDA_CHAIN_MAXOBS];
    float sigma;
    const float* y;         /* device, [k] */
} sda_chain_obs;
typedef struct {
    sda_chain_model model;
    const float* x_in;
    int64_t in_sp;
    const int32_t* anc;     /* NULL: particle j reads x_in[j] */
    float* out;
    int64_t out_st, out_sp;
    int32_t every;
    int32_t m, transitions;
    uint64_t seed;
    int64_t row0, draw0;
    const sda_chain_obs* obs;   /* HOST pointer; NULL: no weights */
    float* logw;
    float* pmax;
} sda_chain_adv;
int sda_chain_advance(const sda_chain_adv* a, void* stream);
int sda_chain_log_prob(const sda_chain_model* model, const float* x, int b, int len, int64_t sb, int64_t sl, double* out, void* stream);
int sda_bpf_logweights(const float* x, int m, int64_t sp, int d, const sda_chain_obs* obs, float* logw, float* pmax, void* stream);
int sda_bpf_logweights_blocks(int m);
int sda_bpf_cdf(const float* logw, int m, const float* pmax, int npmax, float* w, double* cdf, int32_t* status, void* stream);
int sda_bpf_resample(const double* cdf, int m, uint64_t seed, int64_t obs_index, int32_t* anc, void* stream);
int sda_bpf_traceback(const float* S, int64_t s_st, int64_t s_sp, const int32_t* anc, int m, int n_obs, int step, int d, float* out,
                      void* stream);

/* ------------------------------------------------------------------------------------------
 * Adjoint of the Markov chains (csrc/chain.hip; additive, ABI stays v14): what sda_amd.chains(grad='device') and
 * experiments.lorenz.log_prior(grad='device') launch.  First order, fp32, gather form: every output element is written once by the
 * lane that owns it, there are NO atomics, so a result is bitwise reproducible and the row of a particle (the gradient of a
 * trajectory) does not depend on m (on b) or on the other rows.
 *
 * sda_chain_advance_vjp: gx[j] = (d sda_chain_advance / d x_in[j])^T g for all three kinds, ONE launch that walks the transitions
 *   last to first.  Transition t starts from x_in (t = 0) or from states[(t - 1) * st_st + j * st_sp]: `states` is the forward's
 *   every = 1 output addressed by the forward's strides (its last frame is not read; NULL is allowed when transitions == 1).  Noise
 *   is additive: it is inside the stored states and absent from the Jacobian, so no seed is taken.  every = 1: g is
 *   [transitions][m][d] (strides g_st / g_sp) and the running cotangent after transition t is g[t - 1] + J_t^T (running); every = 0:
 *   g is [m][d], the cotangent of the last state.  An RK4 sub-step is reversed by recomputing its four stage points v_i and
 *   applying J_f(v_i)^T; with model.steps > 1 the states inside a transition are recomputed from its start
 *   state, the prefix again for every sub-step (O(steps^2) on d floats, any steps >= 1).  Geometry as sda_chain_advance: one particle
 *   per lane with state and cotangent in registers (Lorenz-63, Lotka-Volterra: the Jacobian reuses the stage point's expf), or one
 *   component per lane of a sub-group (Lorenz-96: (J^T g)_j = g_{j+1} x_{j+2} - g_{j-2} x_{j-1} + g_{j-1} (x_{j-2} - x_{j+1}) - g_j
 *   by four more shuffles per stage).  anc != NULL (the particle filter's gather) is not differentiated: SDA_E_UNSUPPORTED.
 * sda_chain_log_prob_grad: out[b] exactly as sda_chain_log_prob writes it, and grad[b][i][c] (contiguous, fp32) = d out[b] /
 *   d x[b][i][c] = J_T(x_i)^T r_i - r_{i-1} with r_i = (x_{i+1} - T(x_i)) / noise_std^2, r_{-1} = 0 and no pair at i = len - 1; one
 *   launch.  Kinds 0 and 1, as sda_chain_log_prob.  The upstream cotangent of out[b] is NOT an argument: the caller scales
 *   grad[b] (one multiply), which keeps the kernel's result independent of what is done with the value.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    sda_chain_model model;
    const float* x_in;      /* [m][d], particle stride in_sp */
    int64_t in_sp;
    const int32_t* anc;     /* must be NULL */
    const float* states;    /* the forward's every = 1 output; NULL allowed when transitions == 1 */
    int64_t st_st, st_sp;
    const float* g;         /* output cotangent */
    int64_t g_st, g_sp;
    int32_t every;
    int32_t m, transitions;
    float* gx;              /* [m][d], particle stride gx_sp */
    int64_t gx_sp;
} sda_chain_vjp;
int sda_chain_advance_vjp(const sda_chain_vjp* a, void* stream);
int sda_chain_log_prob_grad(const sda_chain_model* model, const float* x, int b, int len, int64_t sb, int64_t sl, double* out,
                            float* grad, void* stream);

/* ------------------------------------------------------------------------------------------
 * Kolmogorov flow (csrc/kflow.hip; additive, ABI stays v14): the simulator behind sda/mcs.py:244-338.  The reference only CALLS
 * jax-cfd, so the scheme (tests/kflow_ref.py) is this project's restatement of semi_implicit_navier_stokes
 * with its defaults: faithful, not pinned to a reference output.
 *
 * State: fields [2][n][n] fp32 (u, v staggered; axis 0 of a plane is x), field stride in floats given per call, planes and rows
 * contiguous.  n % 16 == 0, 16 <= n <= 512 (sda_kflow_serves), at most 65535 fields per call.
 * sda_kflow_explicit: out[b] = (u*, v*) = x[b] + delta (-adv + nu lap + f), out contiguous [nb][2][n][n].
 * sda_kflow_hartley: nb planes [n][n]; side 0: out = Hm x; side 1: out = (x Hm) o scale (scale [n][n] or NULL); out contiguous, out != x.
 * sda_kflow_project: out[b] = x[b] - grad(lap^-1 div x[b]) (the mean mode of the potential is 0); work: 2 nb n n floats; out may be x.
 * sda_kflow_advance: `transitions` transitions of model.steps sub-steps each, all queued, nothing read back.  every = 0: out[b] (field
 *   stride 2 n n) = the last state; every = 1: out[t * out_st + b * 2 n n] = the state after transition t.  work:
 *   sda_kflow_work_floats(n, nb) floats.  x is only read.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t n, steps;
    float delta;            /* dt / steps, rounded to fp32 */
    float nu;               /* 1 / reynolds */
    const float* hm;        /* device [n][n]: (cos(2 pi a b / n) + sin(2 pi a b / n)) / sqrt(n) */
    const float* inv;       /* device [n][n]: 1 / (lam_a + lam_b), lam_k = (2 cos(2 pi k / n) - 2) / h^2; 0 at [0][0] */
    const float* forcing;   /* device [n]: sin(4 (j + 1/2) h) */
} sda_kflow_model;
int sda_kflow_serves(int n);
int64_t sda_kflow_work_floats(int n, int nb);
int sda_kflow_explicit(const sda_kflow_model* m, const float* x, int64_t x_sb, int nb, float* out, void* stream);
int sda_kflow_hartley(const float* hm, int n, const float* x, int64_t x_sb, int nb, int side, const float* scale, float* out,
                      void* stream);
int sda_kflow_project(const sda_kflow_model* m, const float* x, int64_t x_sb, int nb, float* out, int64_t out_sb, float* work,
                      void* stream);
int sda_kflow_advance(const sda_kflow_model* m, const float* x, int64_t x_sb, int nb, int transitions, int every, float* out,
                      int64_t out_st, float* work, void* stream);

/* ------------------------------------------------------------------------------------------
 * Adjoint of the Kolmogorov-flow sub-step (csrc/kflow.hip; additive, ABI stays v14).  The projection is its own transpose
 * (G = -D^T, L and Hm symmetric), so sda_kflow_project is also its adjoint; what is added is the vector-Jacobian product of
 * sda_kflow_explicit and the schedule that walks one transition backwards.  Derivative conventions at the limiter's kinks are
 * those of torch autograd on the torch-ops route.  Gather form, no atomics: bitwise reproducible.
 * sda_kfvjp_explicit: out[b] = (d explicit / dx at x[b])^T g[b]; x, g strided fields, out contiguous [nb][2][n][n], out != x, g.
 * sda_kfvjp_transition: out[b] = (d transition / dx0 at x0[b])^T g[b].  Recomputes the model.steps - 1 inner sub-step states from
 *   x0 with the forward launches (bitwise the forward pass's), then per sub-step, last to first, g <- P g (four launches) and
 *   g <- E'(x_s)^T g (one).  All queued, nothing read back.  g_sb % 4 == 0, g 16-byte aligned; out contiguous, out != x0 (out may
 *   be g).  work: sda_kfvjp_work_floats(n, nb, steps) = (steps + 2) 2 nb n n floats (0: not served).
 * ------------------------------------------------------------------------------------------ */
int64_t sda_kfvjp_work_floats(int n, int nb, int steps);
int sda_kfvjp_explicit(const sda_kflow_model* m, const float* x, int64_t x_sb, const float* g, int64_t g_sb, int nb, float* out,
                       void* stream);
int sda_kfvjp_transition(const sda_kflow_model* m, const float* x0, int64_t x0_sb, const float* g, int64_t g_sb, int nb, float* out,
                         float* work, void* stream);

/* ------------------------------------------------------------------------------------------
 * Linear-Gaussian state space (csrc/lgss.hip; additive, ABI stays v14): the DampedSpring of sda/mcs.py:60-82 and any chain
 *   x_0 ~ N(m0, P0),  x_{i+1} = A x_i + b + w_i, w_i ~ N(0, Q),  y = H x + c + v, v ~ N(0, sigma^2 I_k),   1 <= d, k <= 8,
 * its exact posterior given N observations `step` transitions apart (time index i = 0 .. T = (N - 1) step, observation j at
 * i = j step, (m0, P0) the law of the state at i = 0) and the exact eps of the VP-noised trajectory.  Matrices travel BY VALUE.
 *
 * sda_lgss_advance (fp32): m states [m][d] (stride in_sp), `transitions` >= 1 in ONE launch; every / out_st / out_sp as in
 *   sda_chain_advance.  x'[i] = b[i] + sum_j A[i][j] x[j] accumulated in index order with fma, then + sum_{j<=i} Lq[i][j] z[j] the
 *   same way (Lq: lower Cholesky factor of Q).  z of state j at transition t is BY DEFINITION row j of
 *   sda_randn_rows(out[m][d], seed, row0, draw = draw0 + t).  One state per lane, state in registers.
 * sda_lgss_tables (HOST only, float64, no device access): table[i] for i = 0 .. T, sda_lgss_table_doubles(d, k, T) doubles in all,
 *   each slab {K_i[d][k], G_i[d][d], L_i[d][d], Ls_i[k][k], logdet_i}: the Kalman gain (0 where nothing is observed), the backward
 *   gain G_i = P_i A^T (A P_i A^T + Q)^-1 (0 at i = T), the lower Cholesky factor of P_i - G_i A P_i (of P_T at i = T), the lower
 *   factor of the innovation covariance H P_i^- H^T + sigma^2 I and its log-determinant (0 where nothing is observed).  Both
 *   covariance updates use the Joseph form and are symmetrised.  SDA_E_BADARG if Q, P0 or any factor is not positive definite.
 * sda_lgss_filter: y[B][N][k] fp32 (device) -> mean[B][T+1][d] and logz[B] = log p(y) = sum_j log N(y_j; H m_j^- + c, S_j)
 *   (2 pi terms included), float64, one sequence per lane; `table` is the device copy of sda_lgss_tables' output.
 * sda_lgss_sample: out[B][M][T+1][d] fp32, M exact posterior trajectories per sequence: x_T = mean_T + L_T z_T, then downwards
 *   x_i = mean_i + G_i (x_{i+1} - A mean_i - b) + L_i z_i in float64.  z of sample (b, r) at time i = row b M + r of
 *   sda_randn_rows(out[B M][d], seed, row0, draw = draw0 + i): it depends on neither the launch geometry nor M' > r, B' > b.
 *   One sample per lane; a tile of times is staged in LDS and written as contiguous rows.
 * sda_lgss_score_factor / sda_lgss_score: with Lambda the block-tridiagonal precision of (x_0 .. x_T) (diagonal blocks
 *   P0^-1 + A^T Q^-1 A, Q^-1 + A^T Q^-1 A, .., Q^-1; off-diagonal -A^T Q^-1) and m its mean, x(t) ~ N(mu m, mu^2 Lambda^-1 +
 *   sigma^2 I) and eps = sigma Lambda (mu^2 I + sigma^2 Lambda)^-1 (x - mu m).  `prec` (device, float64,
 *   sda_lgss_score_doubles(d, T, 0) values) = {P0^-1, Q^-1, A^T Q^-1, A^T Q^-1 A, m[T+1][d]}; coef (device, fp32) = {mu, sigma}.
 *   factor: one wave, block Cholesky (block Thomas order) of mu^2 I + sigma^2 Lambda into work (sda_lgss_score_doubles(d, T, 1)
 *   doubles).  score: x[n][T+1][d] fp32 -> out likewise, one trajectory per lane, float64 sweeps, ywork: n (T+1) d doubles.
 *   zero_mean != 0 takes m = 0 and mu out of the right-hand side: Lambda and the solve commute, the Jacobian is symmetric, and
 *   this is the vector-Jacobian product on a cotangent x.
 * Bad arguments (null pointers, d or k outside 1..8, T < 0, counts < 1) are refused on the host before any launch.
 * ------------------------------------------------------------------------------------------ */
#define SDA_LGSS_MAXD 8
typedef struct {
    int32_t d;
    float A[SDA_LGSS_MAXD][SDA_LGSS_MAXD];
    float b[SDA_LGSS_MAXD];
    float Lq[SDA_LGSS_MAXD][SDA_LGSS_MAXD];     /* lower Cholesky factor of Q */
} sda_lgss_model;
typedef struct {
    int32_t d, k;
    double A[SDA_LGSS_MAXD][SDA_LGSS_MAXD], b[SDA_LGSS_MAXD], Q[SDA_LGSS_MAXD][SDA_LGSS_MAXD];
    double m0[SDA_LGSS_MAXD], P0[SDA_LGSS_MAXD][SDA_LGSS_MAXD];     /* the law of the state at time index 0 */
    double H[SDA_LGSS_MAXD][SDA_LGSS_MAXD], c[SDA_LGSS_MAXD];       /* H is k x d */
    double sigma;
} sda_lgss_model64;
int sda_lgss_advance(const sda_lgss_model* model, const float* x_in, int64_t in_sp, int m, int transitions, int every, float* out,
                     int64_t out_st, int64_t out_sp, uint64_t seed, int64_t row0, int64_t draw0, void* stream);
int64_t sda_lgss_table_doubles(int d, int k, int T);
int sda_lgss_tables(const sda_lgss_model64* model, int step, int N, double* table);
int sda_lgss_filter(const sda_lgss_model64* model, const double* table, int step, int N, const float* y, int B, double* mean,
                    double* logz, void* stream);
int sda_lgss_sample(const sda_lgss_model64* model, const double* table, const double* mean, int T, int B, int M, uint64_t seed,
                    int64_t row0, int64_t draw0, float* out, void* stream);
int64_t sda_lgss_score_doubles(int d, int T, int which);
int sda_lgss_score_factor(int d, int T, const double* prec, const float* coef, double* work, void* stream);
int sda_lgss_score(int d, int T, const double* prec, const float* coef, const double* work, const float* x, int n, int zero_mean,
                   double* ywork, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Stochastic ensemble Kalman smoother (csrc/enks.hip; additive, ABI stays v14): per observation one gain launch and one update
 * launch, whatever the ensemble size m, the observed components k or the window length.  Ensemble slabs are [m][d] fp32 (member
 * stride in floats given per call, components contiguous); a, z and work are [k][m] fp32 scratch.  One analysis is
 *   step 1  inflation of the observed slab: x_j <- xbar + lambda (x_j - xbar); lambda == 1 touches nothing;
 *   step 2  h_j = (x_j[idx[r]] - shift[r]) / scale[r] (the sda_chain_obs selection), hbar, a_j = h_j - hbar;
 *   step 3  C = sum_j a_j a_j^T / (m - 1) + sigma^2 I, its Cholesky factor and inverse, all float64;
 *   step 4  z_j = C^-1 ((y + sigma eps_j) - h_j), eps_j[r] = element r of row j of sda_randn_rows(.., seed ^ 0x454E4B53, 0, draw);
 *   step 5  for every slab s of the window and component c: p = sum_j (x_j[s][c] - xbar[s][c]) a_j / (m - 1), x_j[s][c] += p . z_j.
 * Every sum over the members is float64 with an order fixed by m alone; no atomics; bitwise reproducible.
 *
 * sda_enks_gain: steps 2 - 4 in ONE launch of one workgroup.  x = the observed slab, read as step 1 WOULD leave it (it is not
 *   written).  status[0] = 0, or 1 when a pivot of the factor is not positive and finite (z is then 0, so the update adds
 *   nothing); read it once, at the end, as sda_bpf_cdf's.
 * sda_enks_update: steps 1 and 5 in ONE launch over the nslab slabs S + s * s_st, one workgroup per slab; the LAST slab is the
 *   observed one and the only one inflated.  A slab's result does not depend on nslab.  Memory outside those slabs is not touched.
 * Served: 2 <= m <= 2^22, 1 <= d <= 64, 1 <= k <= min(d, SDA_CHAIN_MAXOBS); anything else is SDA_E_BADARG / SDA_E_UNSUPPORTED
 * before any launch.
 * ------------------------------------------------------------------------------------------ */
int sda_enks_gain(const float* x, int m, int64_t sp, int d, const sda_chain_obs* obs, float inflation, uint64_t seed, int64_t draw,
                  float* a, float* z, float* work, int32_t* status, void* stream);
int sda_enks_update(float* S, int64_t s_st, int64_t s_sp, int nslab, int m, int d, int k, float inflation, const float* a,
                    const float* z, void* stream);

/* ------------------------------------------------------------------------------------------
 * The same smoother solved in ENSEMBLE space (csrc/enks_wide.hip; additive, ABI stays v14), for wide states and a modest
 * ensemble: an m x m system instead of a k x k one, and the observed values H = A(members) come from the caller, so A is any
 * callable.  The ensemble is S [T][m][d] fp32, time-major as above; H, Y, D, eps are [m][k] fp32, member-major, k contiguous;
 * W is [m][m] fp32.  It is the analysis above reordered:
 *   step 1  inflation of the observed slab: x_j <- x_j + (lambda - 1)(x_j - xbar), xbar summed in float64 in member order and
 *           rounded to fp32; lambda == 1 touches nothing (sda_enkw_transform, mode 1, a launch of its own BEFORE H is formed);
 *   step 2  hbar = the member mean of H, float64, member order; Y = H - hbar (fp32); D_j = (y + sigma eps_j) - h_j (fp32),
 *           eps_j = row j of sda_randn_rows(.., seed ^ 0x454E4B53, 0, draw): the perturbations of sda_enks_gain;
 *   step 3  G = Y Y^T, B = Y D^T, both m x m, contracted over k in float64 (products of fp32 operands are exact there);
 *   step 4  W = (G / (m - 1) + sigma^2 I)^-1  B / (m - 1) by a float64 Cholesky factor, stored fp32;
 *   step 5  for every slab s of the window and component c: x_j[s][c] += sum_m W[m][j] (x_m[s][c] - xbar[s][c]), xbar in
 *           float64 in member order, the centred values rounded to fp32, the product an fp32 fma chain in member order on
 *           the matrix cores; it is formed on the centred values only (1^T W = 0 holds analytically, not in rounding).
 * By the push-through identity Y^T (Y Y^T / (m - 1) + sigma^2 I)^-1 = (Y^T Y / (m - 1) + sigma^2 I)^-1 Y^T this is steps 1 - 5
 * above exactly.  Four launches per analysis (five with inflation) whatever m, k, d and the window; no atomics, nothing read
 * back, no workgroup waits for another; bitwise reproducible; a slab's result does not depend on the other slabs of a launch.
 *
 * sda_enkw_prepare: step 2.  eps may be NULL.
 * sda_enkw_gram: step 3, split over k into chunks of 512: part holds sda_enkw_gram_doubles(m, k) doubles, per chunk the
 *   [pad16(m)][2 pad16(m)] partial of [G | B] (v_mfma_f64_16x16x4_f64; rows past m and values past k enter as zeros).
 * sda_enkw_solve: step 4 in one workgroup: sums the partials in chunk order, factors, solves (bwork: m x m doubles of
 *   scratch), writes W and status[0] = 0, or 1 when a pivot is not positive and finite or an entry of W is not finite; W is
 *   then all zeros, so the transform adds nothing.  Read the status once, at the end.
 * sda_enkw_transform: mode 0 is step 5 in place over the nslab slabs S + s * s_st (grid: tiles of 128 components x slabs;
 *   v_mfma_f32_16x16x4_f32); mode 1 is step 1 on those slabs (W unused).  Memory outside those slabs is not touched.
 * Served: 2 <= m <= 128, 1 <= k <= 2^24, d >= 1 with member stride s_sp >= d, nslab <= 65535, fp32; anything else is
 * SDA_E_BADARG / SDA_E_UNSUPPORTED before any launch.
 * ------------------------------------------------------------------------------------------ */
int64_t sda_enkw_gram_doubles(int m, int k);
int sda_enkw_prepare(const float* H, int m, int k, const float* y, float sigma, uint64_t seed, int64_t draw, float* Y, float* D,
                     float* eps, void* stream);
int sda_enkw_gram(const float* Y, const float* D, int m, int k, double* part, void* stream);
int sda_enkw_solve(const double* part, int m, int k, float sigma, double* bwork, float* W, int32_t* status, void* stream);
int sda_enkw_transform(float* S, int64_t s_st, int64_t s_sp, int nslab, int m, int64_t d, const float* W, float inflation, int mode,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * The ensemble-space smoother LOCALISED by domain (csrc/enks_local.hip; additive, ABI stays v14): R-localisation as in the LETKF
 * literature, in this project's perturbed-observation form.
 *   Grid and blocks.  The state event is a periodic grid [C][Hg][Wg] (a ring of n components is [1][1][n]), cut into blocks of
 *     bh x bw points, Hg % bh == 0 and Wg % bw == 0; block b = br (Wg / bw) + bc.  All C channels of a block's points share one
 *     weight matrix W[b].  A block's components are numbered q = (channel, row, column inside the block), row-major.
 *   Weights.  Observed value i sits at the real-valued grid position p_i = (row, col).  For block b with centre c_b (the mean of its
 *     points' coordinates) rho_{b,i} = GC(dist(c_b, p_i) / radius), dist the periodic Euclidean distance on the Hg x Wg torus and GC
 *     the Gaspari-Cohn fifth-order function, of support 2 radius:
 *       0 <= z <= 1:  -z^5/4 + z^4/2 + 5 z^3/8 - 5 z^2/3 + 1
 *       1 <  z <  2:   z^5/12 - z^4/2 + 5 z^3/8 + 5 z^2/3 - 5 z + 4 - 2/(3 z)
 *       otherwise 0.
 *   Plan.  Positions are fixed for a run, so the lists are built once, on the host, in float64, and uploaded as a CSR table:
 *     offsets[nblk + 1], idx[nnz] int32 ascending inside a block, rho[nnz] rounded to fp32; only entries whose fp32 value is
 *     strictly positive are listed.  (The library takes the table; sda_amd.ops.enkl_plan builds it.)
 *   Per analysis.  Steps 1 and 2 are sda_enkw_transform (mode 1) and sda_enkw_prepare above, unchanged: the same Y, D and
 *     perturbation stream.  Then for every block b, summed over its listed i in list order:
 *       G_b = sum_i rho_{b,i} Y[:, i] Y[:, i]^T,   B_b = sum_i rho_{b,i} Y[:, i] D[:, i]^T      (float64; rho Y is exact there)
 *       W_b = (G_b / (m - 1) + sigma^2 I)^-1  B_b / (m - 1)                                      (float64 Cholesky, stored fp32)
 *     and for every slab s of the window and component q of the block x_j[s][q] += sum_m W_b[m][j] (x_m[s][q] - xbar[s][q]),
 *     formed as step 5 above.  With every rho = 1 and one block this is the analysis above; a block with an empty list has
 *     W_b = 0 and is not touched.
 * sda_enkl_pack: T [k][2 m] fp32, T[i] = (Y[:, i] | D[:, i]), so a gathered observed value is 2 m contiguous floats.
 * sda_enkl_weights: one workgroup per block: [G_b | B_b] on v_mfma_f64_16x16x4_f64 over the list, the factor in LDS (m^2 doubles:
 *   m <= 128), the solve; bwork: nblk m^2 doubles of scratch; W [nblk][m][m] fp32; status[b] = 0, or 1 when a pivot is not
 *   positive and finite, an entry of W[b] is not finite or an index is outside 0 .. k - 1 (it is then not read); W[b] is then
 *   all zeros, and no other block is affected.  Read the status once, at the end.
 * sda_enkl_transform: grid (blocks x tiles of 128 block components, slabs), in place over the nslab slabs S + s * s_st, member
 *   stride s_sp >= C Hg Wg; v_mfma_f32_16x16x4_f32.  A block with an empty list is skipped without a load.  Memory outside
 *   those slabs is not touched.
 * Three launches per analysis after prepare; no atomics, nothing read back, no workgroup waits for another; bitwise
 * reproducible; a block's result depends on its own list alone and a slab's on m, the block and W[b] alone.
 * Served: 2 <= m <= 128, 1 <= k <= 2^24, nblk <= 2^22, nslab <= 65535, fp32, periodic grids only; anything else is
 * SDA_E_BADARG / SDA_E_UNSUPPORTED before any launch.  The analysis is discontinuous across block edges (no interpolation of
 * the weights between blocks), and there is no localisation in time.
 * ------------------------------------------------------------------------------------------ */
int sda_enkl_pack(const float* Y, const float* D, int m, int k, float* T, void* stream);
int sda_enkl_weights(const float* T, int m, int k, const int32_t* offsets, const int32_t* idx, const float* rho, int nblk, float sigma,
                     double* bwork, float* W, int32_t* status, void* stream);
int sda_enkl_transform(float* S, int64_t s_st, int64_t s_sp, int nslab, int m, int C, int Hg, int Wg, int bh, int bw,
                       const int32_t* offsets, const float* W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDA_HIP_H */
