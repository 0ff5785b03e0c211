// The two forward whole-MLP kernels of csrc/mlp1d.hip (see its header), as text that file includes once per value of ML_WF = the D fragments
// that hold a row's window values in window mode: 1 (a window of at most 16 values) and 2 (17 .. 32: Lorenz k = 3, 4).  The including file
// names the kernels (ML_K_FWD, ML_K_FWD_WIDE).  The two input-VJP kernels are csrc/mlp1d_vjp_kernels.hpp, which mlp1d.hip includes right
// behind this text and csrc/mlp_train.hip includes once more.  Text, not a template parameter or a shared body function: the kernels of
// ML_WF = 1 must stay the code they were (tests/test_isa_guard_mlp.py pins their instruction counts; against the one-fragment version the
// window kernels differ in scalar register names and the operand order of four v_add_f32), and a body function the kernels forward to
// compiles to up to 600 instructions more per kernel.  ML_WF matters under `if constexpr (WIN)` only.
// ------------------------------------------------------------------------------------------------------------ forward
template <bool WIN>
__global__ __launch_bounds__(256) void ML_K_FWD(const sda_mlp_desc d, const sda_mlp_win w) {
    extern __shared__ __attribute__((aligned(16))) float ml_lds[];         // two slab buffers
    MlCtx c;
    ml_ctx(c, d);
    ML_T0();
    MlStage st;
    // slab 0 -> buffer 0
    st.src = ml_rsrc(d.w + d.w_off[0]); st.toff = 16u * c.tid;
    st.dst = reinterpret_cast<ml_f32x4*>(ml_lds) + c.tid;
    st.npieces = ml_slab_floats(d.in_f[0], d.out_f[0]) / ML_PIECE;
    for (int p = 0; p < st.npieces; ++p) { ml_f32x4 t[4]; st.issue(t, p); st.commit(t, p); }
    // every GEMM's bias -> LDS, once (read per GEMM as the C operand of its first MFMAs: from global memory each first MFMA waited a
    // full L2 round trip -- 14 x ~2 000 cycles of a tile's 120 000 in the GEMM phase)
    float* const bl = ml_lds + 2 * ML_SLAB;
    {
        const int nb = d.b_off[d.ngemm - 1] + 16 * ml_mf(d.out_f[d.ngemm - 1]);
        for (int i = c.tid; i < nb; i += 256) bl[i] = d.bias[i];
    }
    ml_f32x4 h[8], a[8], acc[8], zs[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) zs[m] = ml_f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (WIN) {
        // (inline copy of ml_win_load, see there)  row (b, i): features [0, WC) = x[b][i .. i + 2k][:] -- WC consecutive floats of the trajectory --, then the time embedding
        const MlWinRow wr = ml_win_row(w, c);
        const int wc = (w.len - w.nw + 1) * w.c;
        const float* xr = w.x + ((int64_t)wr.b * w.len + wr.i) * w.c;
#pragma unroll
        for (int m = 0; m < 8; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = 16 * m + 4 * c.kq + r;
                const bool isx = f < wc, ise = !isx && f < wc + w.emb_n;
                const float xv = xr[isx ? f : 0], ev = w.emb[ise ? f - wc : 0];
                a[m][r] = !c.rowok ? 0.f : (isx ? xv : (ise ? ev : 0.f));
            }
    } else {
        ml_load_rows(d.x, d.x_ld, d.in_f[0], c, a);
    }
    __syncthreads();
    ML_STAMP(0);                                           // first slab + input rows
    const bool silu = d.act == SDA_ACT_SILU;
    int rb = 0;                                            // residual-block counter (index into the saves)
    MlMeta mc = ml_meta(d, 0), mn = ml_meta(d, 1);
    for (int g = 0; g < d.ngemm; ++g) {
        const MlMeta mm = ml_meta(d, g + 2);
        const float* wl = ml_lds + (g & 1) * ML_SLAB;
        const bool last = g + 1 == d.ngemm;
        st.src = ml_rsrc(d.w + (last ? 0 : mn.w_off)); st.toff = 16u * c.tid;
        st.dst = reinterpret_cast<ml_f32x4*>(ml_lds + ((g + 1) & 1) * ML_SLAB) + c.tid;
        st.npieces = last ? 0 : ml_slab_floats(mn.in_f, mn.out_f) / ML_PIECE;
        const int mf = ml_mf(mc.out_f), cw = mc.in_f;
        // the bias is the C operand of the GEMM's first MFMAs: loaded here, long before it is needed
        ml_f32x4 bias[8];
        {
            const float* bg = bl + mc.b_off + 4 * c.kq;
#pragma unroll
            for (int m = 0; m < 8; ++m) bias[m] = m < mf ? *reinterpret_cast<const ml_f32x4*>(bg + 16 * m) : ml_f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if (mc.kind == 1) {
            // ---- residual block, first half: save a; h = LN(a)
            const float inv_c = 1.f / (float)cw, inv_v = 1.f / (float)(d.unbiased ? cw - 1 : cw);
            float mean, rstd;
            auto ln = [&](auto FULL_) { ml_ln<decltype(FULL_)::value>(a, h, cw, c, inv_c, inv_v, d.eps, mean, rstd); };
            if (cw == 128) ln(std::true_type{});
            else ln(std::false_type{});
            if (d.mean_save && c.kq == 0 && c.rowok) {
                d.mean_save[(int64_t)rb * d.stat_stride + c.row] = mean;
                d.rstd_save[(int64_t)rb * d.stat_stride + c.row] = rstd;
            }
            ML_STAMP(3);                                   // a_save, LayerNorm
        }
        ML_STAMP(1);                                       // GEMM set-up (stage descriptor, bias fragments)
        // the save streams ride the 128 -> 128 multiplies (one store per K quad, see ml_mm): the block input under the block's first
        // multiply, the pre-activation -- a copy, the accumulators are rewritten -- under its second; other widths store in the epilogue
        const bool ride = d.z_save && cw == 128 && c.rowok;
        if (mc.kind == 0) ml_gemm(wl, mc.in_f, mc.out_f, a, acc, bias, st, c, nullptr, a);
        else if (mc.kind == 1)
            ml_gemm(wl, mc.in_f, mc.out_f, h, acc, bias, st, c,
                    ride ? d.a_save + (int64_t)rb * d.save_stride + c.row * d.save_ld + 4 * c.kq : nullptr, a);
        else
            ml_gemm(wl, mc.in_f, mc.out_f, h, acc, bias, st, c,
                    ride ? d.z_save + (int64_t)rb * d.save_stride + c.row * d.save_ld + 4 * c.kq : nullptr, zs);
        ML_STAMP(2);                                       // GEMM (+ staging)
        __syncthreads();                                   // slab hand-off: the next slab is complete, this one is free
        ML_STAMP(5);                                       // hand-off barrier
        if (mc.kind == 0) {
#pragma unroll
            for (int m = 0; m < 8; ++m) a[m] = acc[m];
        } else if (mc.kind == 1) {
            // z = W1 LN(a) + b1 (saved); h = act(z)
            // the saves (block input a, pre-activation z) go out HERE, behind the GEMM whose slab staging has just completed: vmcnt
            // retires in order, so a store issued in front of staging loads makes the wait for those loads a wait for the store's
            // round trip to HBM (the block input written before the GEMM cost the forward ~20 %)
            if (d.z_save && c.rowok && mc.out_f != 128) {
                float* zp = d.z_save + (int64_t)rb * d.save_stride + c.row * d.save_ld + 4 * c.kq;
                float* as = d.a_save + (int64_t)rb * d.save_stride + c.row * d.save_ld + 4 * c.kq;
#pragma unroll
                for (int m = 0; m < 8; ++m)
                    if (m < mf) {
                        *reinterpret_cast<ml_f32x4*>(zp + 16 * m) = acc[m];
                        *reinterpret_cast<ml_f32x4*>(as + 16 * m) = a[m];
                    }
            }
#pragma unroll
            for (int m = 0; m < 8; ++m) zs[m] = acc[m];
            auto epi = [&](auto SILU_) {
#pragma unroll
                for (int m = 0; m < 8; ++m)
#pragma unroll
                    for (int r = 0; r < 4; ++r) h[m][r] = decltype(SILU_)::value ? sda_act(SDA_ACT_SILU, acc[m][r]) : sda_act(d.act, acc[m][r]);
            };
            if (silu) epi(std::true_type{});
            else epi(std::false_type{});
        } else {
#pragma unroll
            for (int m = 0; m < 8; ++m) a[m] += acc[m];
            ++rb;
        }
        ML_STAMP(4);                                       // epilogue
        mc = mn; mn = mm;
    }
    if constexpr (WIN) ml_win_fold<ML_WF>(w, c, a);
    else ml_store_rows(d.out, d.out_ld, d.out_f[d.ngemm - 1], c, a);
    ML_STAMP(6);                                           // output
    ML_DUMP();
}

template <bool WIN>
__global__ __launch_bounds__(256) void ML_K_FWD_WIDE(const sda_mlp_desc d, const sda_mlp_win w) {
    extern __shared__ __attribute__((aligned(16))) float ml_lds[];         // two unit buffers + the biases
    MlCtx c;
    ml_ctx(c, d);
    MlMeta mc = ml_meta(d, 0), mn = ml_meta(d, 1);
    MlStage st;
    st.src = ml_rsrc(d.w + mc.w_off); st.toff = 16u * c.tid;
    st.dst = reinterpret_cast<ml_f32x4*>(ml_lds) + c.tid;
    st.npieces = mlw_unit_floats(mc.in_f, mc.out_f) / ML_PIECE;
    for (int p = 0; p < st.npieces; ++p) { ml_f32x4 t[4]; st.issue(t, p); st.commit(t, p); }
    float* const bl = ml_lds + 2 * ML_SLAB;
    {
        const int nb = d.b_off[d.ngemm - 1] + 16 * mlw_mf(d.out_f[d.ngemm - 1]);
        for (int i = c.tid; i < nb; i += 256) bl[i] = d.bias[i];
    }
    // a = the residual stream, h = a GEMM's input, acc = its output: 3 x 64 registers (+ 64 of A fragments and the staging ones)
    ml_f32x4 h[16], a[16], acc[16];
    if constexpr (WIN) ml_win_load(w, c, a);
    else ml_load_rows(d.x, d.x_ld, d.in_f[0], c, a);
    __syncthreads();
    const bool silu = d.act == SDA_ACT_SILU;
    int rb = 0, buf = 0;
    for (int g = 0; g < d.ngemm; ++g) {
        const MlMeta mm = ml_meta(d, g + 2);
        const bool last = g + 1 == d.ngemm;
        const int cw = mc.in_f;
        if (mc.kind == 1) {
            const float inv_c = 1.f / (float)cw, inv_v = 1.f / (float)(d.unbiased ? cw - 1 : cw);
            float mean, rstd;
            if (cw == 256) ml_ln<true>(a, h, cw, c, inv_c, inv_v, d.eps, mean, rstd);
            else ml_ln<false>(a, h, cw, c, inv_c, inv_v, d.eps, mean, rstd);
            if (d.mean_save && c.kq == 0 && c.rowok) {
                d.mean_save[(int64_t)rb * d.stat_stride + c.row] = mean;
                d.rstd_save[(int64_t)rb * d.stat_stride + c.row] = rstd;
            }
        } else if (mc.kind == 0) {
#pragma unroll
            for (int m = 0; m < 16; ++m) h[m] = a[m];
        }
        mlw_gemm(ml_lds, buf, d.w + mc.w_off, mc.in_f, mc.out_f, d.w + (last ? 0 : mn.w_off),
                 last ? 0 : mlw_unit_floats(mn.in_f, mn.out_f) / ML_PIECE, h, acc, st, c);
        {
            // + the bias, from LDS (as the C operand of the first MFMAs, the narrow kernel's way, its 32 registers come on top of a, h, acc and
            // the A fragments: spills)
            const float* bg = bl + mc.b_off + 4 * c.kq;
            const int nm = mlw_mf(mc.out_f);
#pragma unroll
            for (int m = 0; m < 16; ++m)
                if (m < nm) acc[m] += *reinterpret_cast<const ml_f32x4*>(bg + 16 * m);
        }
        if (mc.kind == 0) {
#pragma unroll
            for (int m = 0; m < 16; ++m) a[m] = acc[m];
        } else if (mc.kind == 1) {
            // z = W1 LN(a) + b1; both saved streams leave here, behind the GEMM (see the narrow kernel); h = act(z)
            if (d.z_save && c.rowok) {
                const int nm = mlw_mf(mc.out_f);
                float* zp = d.z_save + (int64_t)rb * d.save_stride + c.row * d.save_ld + 4 * c.kq;
                float* as = d.a_save + (int64_t)rb * d.save_stride + c.row * d.save_ld + 4 * c.kq;
#pragma unroll
                for (int m = 0; m < 16; ++m)
                    if (m < nm) {
                        *reinterpret_cast<ml_f32x4*>(zp + 16 * m) = acc[m];
                        *reinterpret_cast<ml_f32x4*>(as + 16 * m) = a[m];
                    }
            }
            auto epi = [&](auto SILU_) {
#pragma unroll
                for (int m = 0; m < 16; ++m) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) h[m][r] = decltype(SILU_)::value ? sda_act(SDA_ACT_SILU, acc[m][r]) : sda_act(d.act, acc[m][r]);
                    // (64 independent chains: left free, the scheduler interleaves them all and their temporaries spill)
                    if (m & 1) __builtin_amdgcn_sched_barrier(0);
                }
            };
            if (silu) epi(std::true_type{});
            else epi(std::false_type{});
        } else {
#pragma unroll
            for (int m = 0; m < 16; ++m) a[m] += acc[m];
            ++rb;
        }
        mc = mn; mn = mm;
    }
    if constexpr (WIN) ml_win_fold<ML_WF>(w, c, a);
    else ml_store_rows(d.out, d.out_ld, d.out_f[d.ngemm - 1], c, a);
}
