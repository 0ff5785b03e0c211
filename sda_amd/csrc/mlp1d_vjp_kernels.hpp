// The two input-VJP kernels of the whole MLP, as text (see csrc/mlp1d_kernels.hpp for why text).  ONE text, three inclusions: csrc/mlp1d.hip
// includes it behind the forward text, once per ML_WF, as mlp_bwd_kernel / mlp_bwd_kernel_wide and mlp_win2_bwd / mlp_win2_bwd_wide;
// csrc/mlp_train.hip includes it with ML_WF = 1 as mlp_train_vjp_kernel / mlp_train_vjp_kernel_wide (<false> only), the VJP that also stores
// the cotangent streams.  Next to ML_WF and the names ML_K_BWD, ML_K_BWD_WIDE the including file defines three hooks:
//   ML_VJP_ARGS        the kernels' parameter list;
//   ML_VJP_ENTRY       whatever else must be in scope behind it: the text names `d` (sda_mlp_desc) and, under `if constexpr (WIN)`, `w`
//                      (sda_mlp_win).  Empty where both are parameters;
//   ML_COT(g, n, v)    the fragments v hold the cotangent at GEMM g's output, n features wide.  Stands behind the hand-off barrier, as the
//                      forward's saves do.  A no-op in mlp1d.hip.
// d.w = the slabs of the TRANSPOSED matrices (backward GEMM of forward GEMM g: out_f[g] -> in_f[g], no bias), same offsets table;
// x = cotangent rows (width out_f[last]), out = input-gradient rows (width in_f[0]); the GEMM list is walked backwards.
template <bool WIN>
__global__ __launch_bounds__(256) void ML_K_BWD(ML_VJP_ARGS) {
    extern __shared__ __attribute__((aligned(16))) float ml_lds[];
    ML_VJP_ENTRY
    MlCtx c;
    ml_ctx(c, d);
    const int gl = d.ngemm - 1;
    MlStage st;
    st.src = ml_rsrc(d.w + d.w_off[gl]); st.toff = 16u * c.tid;
    st.dst = reinterpret_cast<ml_f32x4*>(ml_lds) + c.tid;
    st.npieces = ml_slab_floats(d.out_f[gl], d.in_f[gl]) / ML_PIECE;
    for (int p = 0; p < st.npieces; ++p) { ml_f32x4 v[4]; st.issue(v, p); st.commit(v, p); }
    ml_f32x4 h[8], gacc[8], acc[8], zero[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) zero[m] = ml_f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (WIN) {
        // (inline copy of ml_win_cot, see ml_win_load)  the cotangent of the window outputs = fold's adjoint of cn ghat: slot j of window (b, i) receives ghat[b][i + j] where fold reads it
        const MlWinRow wr = ml_win_row(w, c);
        const int k = (w.len - w.nw) / 2, wc = (2 * k + 1) * w.c;
#pragma unroll
        for (int m = 0; m < 8; ++m) gacc[m] = ml_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < ML_WF; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = 16 * m + 4 * c.kq + r, fc = f < wc ? f : 0;
                const int j = fc / w.c, ch = fc - j * w.c;
                const bool sel = c.rowok && f < wc && ml_win_sel(wr, j, k);
                const float gv = w.ghat[sel ? ((int64_t)wr.b * w.len + wr.i + j) * w.c + ch : 0];
                gacc[m][r] = sel ? gv * w.cn : 0.f;
            }
    } else {
        ml_load_rows(d.x, d.x_ld, d.out_f[gl], c, gacc);
    }
    __syncthreads();
    const bool silu = d.act == SDA_ACT_SILU;
    int rb = 0;
    for (int g = 0; g < d.ngemm; ++g) rb += d.kind[g] == 2;
    int buf = 0;
    MlMeta mc = ml_meta(d, gl), mn = ml_meta(d, gl - 1);
    for (int g = gl; g >= 0; --g, buf ^= 1) {
        const MlMeta mm = ml_meta(d, g - 2);
        const float* wl = ml_lds + buf * ML_SLAB;
        const bool last = g == 0;
        st.src = ml_rsrc(d.w + (last ? 0 : mn.w_off)); st.toff = 16u * c.tid;
        st.dst = reinterpret_cast<ml_f32x4*>(ml_lds + (buf ^ 1) * ML_SLAB) + c.tid;
        st.npieces = last ? 0 : ml_slab_floats(mn.out_f, mn.in_f) / ML_PIECE;
        if (mc.kind == 2) --rb;
        // what the epilogue reads from the forward: issued before the multiply
        const int cw = mc.in_f, nm = ml_mf(cw);
        const int64_t srow = c.rowok ? c.row : 0;
        ml_f32x4 sv[8];                                    // kind 2: z; kind 1: the block input a
        float mean = 0.f, rs = 0.f;
        if (mc.kind != 0) {
            const float* sp = (mc.kind == 2 ? d.z_save : d.a_save) + (int64_t)rb * d.save_stride + srow * d.save_ld + 4 * c.kq;
#pragma unroll
            for (int m = 0; m < 8; ++m) sv[m] = m < nm ? *reinterpret_cast<const ml_f32x4*>(sp + 16 * m) : ml_f32x4{0.f, 0.f, 0.f, 0.f};
            if (mc.kind == 1) {
                mean = d.mean_save[(int64_t)rb * d.stat_stride + srow];
                rs = d.rstd_save[(int64_t)rb * d.stat_stride + srow];
            }
        }
        // the multiply's input: the cotangent g itself (Linear; a block's second half) or q (its first half)
        if (mc.kind == 1) ml_gemm(wl, mc.out_f, mc.in_f, h, acc, zero, st, c, nullptr, zero);
        else ml_gemm(wl, mc.out_f, mc.in_f, gacc, acc, zero, st, c, nullptr, zero);
        __syncthreads();
        if (mc.kind != 1) ML_COT(g, mc.out_f, gacc);       // the cotangent this GEMM's output received
        if (mc.kind == 0) {
#pragma unroll
            for (int m = 0; m < 8; ++m) gacc[m] = acc[m];
        } else if (mc.kind == 2) {
            // q = W2^T g, x act'(z)   (features beyond the width: acc = 0 there, so q = 0 x act'(0) = 0)
            auto dact = [&](auto SILU_) {
#pragma unroll
                for (int m = 0; m < 8; ++m)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        h[m][r] = acc[m][r] * (decltype(SILU_)::value ? sda_dact(SDA_ACT_SILU, sv[m][r]) : sda_dact(d.act, sv[m][r]));
            };
            if (silu) dact(std::true_type{});
            else dact(std::false_type{});
            ML_COT(g - 1, cw, h);                          // gz: the cotangent of the block's first GEMM
        } else {
            // gh = W1^T q; g += LN^T(gh) = rstd (gh - mean_c(gh) - x_hat mean'_c(gh x_hat))
            const float inv_c = 1.f / (float)cw, inv_v = 1.f / (float)(d.unbiased ? cw - 1 : cw);
            auto lnb = [&](auto FULL_) { ml_ln_bwd<decltype(FULL_)::value>(sv, acc, gacc, cw, c, inv_c, inv_v, mean, rs); };
            if (cw == 128) lnb(std::true_type{});
            else lnb(std::false_type{});
        }
        mc = mn; mn = mm;
    }
    if constexpr (WIN) {
        // the window part of the input gradient, 16 ML_WF floats per row (the embedding's part is not formed); sda_mc_finish sums the overlaps
        ml_win_gstore<ML_WF>(w, c, gacc);
    } else {
        ml_store_rows(d.out, d.out_ld, d.in_f[0], c, gacc);
    }
}

template <bool WIN>
__global__ __launch_bounds__(256) void ML_K_BWD_WIDE(ML_VJP_ARGS) {
    extern __shared__ __attribute__((aligned(16))) float ml_lds[];
    ML_VJP_ENTRY
    MlCtx c;
    ml_ctx(c, d);
    const int gl = d.ngemm - 1;
    MlMeta mc = ml_meta(d, gl), mn = ml_meta(d, gl - 1);
    MlStage st;
    st.src = ml_rsrc(d.w + mc.w_off); st.toff = 16u * c.tid;
    st.dst = reinterpret_cast<ml_f32x4*>(ml_lds) + c.tid;
    st.npieces = mlw_unit_floats(mc.out_f, mc.in_f) / ML_PIECE;
    for (int p = 0; p < st.npieces; ++p) { ml_f32x4 v[4]; st.issue(v, p); st.commit(v, p); }
    // gacc = the cotangent of the residual stream, h = a GEMM's input, acc = its output
    ml_f32x4 h[16], gacc[16], acc[16];
    if constexpr (WIN) ml_win_cot<ML_WF>(w, c, gacc);
    else ml_load_rows(d.x, d.x_ld, d.out_f[gl], c, gacc);
    __syncthreads();
    const bool silu = d.act == SDA_ACT_SILU;
    int rb = 0, buf = 0;
    for (int g = 0; g < d.ngemm; ++g) rb += d.kind[g] == 2;
    for (int g = gl; g >= 0; --g) {
        const MlMeta mm = ml_meta(d, g - 2);
        const bool last = g == 0;
        if (mc.kind == 2) --rb;
        const int cw = mc.in_f, nm = mlw_mf(cw);
        const int64_t srow = c.rowok ? c.row : 0;
        if (mc.kind != 1) {
#pragma unroll
            for (int m = 0; m < 16; ++m) h[m] = gacc[m];
        }
        mlw_gemm(ml_lds, buf, d.w + mc.w_off, mc.out_f, mc.in_f, d.w + (last ? 0 : mn.w_off),
                 last ? 0 : mlw_unit_floats(mn.out_f, mn.in_f) / ML_PIECE, h, acc, st, c);
        if (mc.kind != 1) ML_COT(g, mc.out_f, gacc);       // the cotangent this GEMM's output received
        // What the epilogue reads from the forward is fetched BEHIND the multiply (in front of it, as the narrow kernel does, its 64 registers
        // would be live under 1024 MFMAs next to gacc, h, acc and the A fragments).  The vector ALU reads the 256 architectural registers
        // only: with gacc, acc and h in them the pre-activations come in groups of four fragments, one group ahead of its use.
        const int64_t soff = (int64_t)rb * d.save_stride + srow * d.save_ld + 4 * c.kq;
        if (mc.kind == 0) {
#pragma unroll
            for (int m = 0; m < 16; ++m) gacc[m] = acc[m];
        } else if (mc.kind == 2) {
            const float* sp = d.z_save + soff;
            // q = W2^T g, x act'(z)   (features beyond the width: acc = 0 there, so q = 0 x act'(0) = 0)
            auto dact = [&](auto SILU_) {
                ml_f32x4 zb[2][4];
                auto fetch = [&](int grp) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        zb[grp & 1][i] = 4 * grp + i < nm ? *reinterpret_cast<const ml_f32x4*>(sp + 16 * (4 * grp + i)) : ml_f32x4{0.f, 0.f, 0.f, 0.f};
                };
                fetch(0);
#pragma unroll
                for (int grp = 0; grp < 4; ++grp) {
                    if (grp < 3) fetch(grp + 1);
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float z = zb[grp & 1][i][r];
                            h[4 * grp + i][r] = acc[4 * grp + i][r] * (decltype(SILU_)::value ? sda_dact(SDA_ACT_SILU, z) : sda_dact(d.act, z));
                        }
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
            if (silu) dact(std::true_type{});
            else dact(std::false_type{});
            ML_COT(g - 1, cw, h);                          // gz: the cotangent of the block's first GEMM
        } else {
            // gh = W1^T q; g += LN^T(gh)
            const float* sp = d.a_save + soff;
            ml_f32x4 sv[16];                               // the block input
#pragma unroll
            for (int m = 0; m < 16; ++m) sv[m] = m < nm ? *reinterpret_cast<const ml_f32x4*>(sp + 16 * m) : ml_f32x4{0.f, 0.f, 0.f, 0.f};
            const float mean = d.mean_save[(int64_t)rb * d.stat_stride + srow], rs = d.rstd_save[(int64_t)rb * d.stat_stride + srow];
            const float inv_c = 1.f / (float)cw, inv_v = 1.f / (float)(d.unbiased ? cw - 1 : cw);
            if (cw == 256) ml_ln_bwd<true>(sv, acc, gacc, cw, c, inv_c, inv_v, mean, rs);
            else ml_ln_bwd<false>(sv, acc, gacc, cw, c, inv_c, inv_v, mean, rs);
        }
        mc = mn; mn = mm;
    }
    if constexpr (WIN) {
        ml_win_gstore<ML_WF>(w, c, gacc);
    } else {
        ml_store_rows(d.out, d.out_ld, d.in_f[0], c, gacc);
    }
}
