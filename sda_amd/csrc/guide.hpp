// THE arithmetic of a Gaussian-guided score evaluation (sda/score.py:387-396) and of the predictor-corrector updates around it
// (score.py:250-261), shared by the unfused kernels (elementwise.hip, observe.hip) and by the epilogues that fuse them into the
// networks (net1d.hpp, mlp1d_common.hpp, step1d.hip): the fused step replays the unfused one operation for operation because both
// call these functions.  The library is built with -ffp-contract=off, so every operation below rounds on its own wherever it is
// inlined; the explicit __f*_rn calls keep the reference's order where a compiler might otherwise pick its own (no fused
// multiply-add, a division per element).  Device code only.
#pragma once
#include "sda_common.hpp"

// ---- per-launch constants
//   eps  = bare ? net : x cx + cn net,  cx = cx0 + cx1 sigma           (an estimator of the form a(t) x + c net(x, t); bare: the network itself)
//   var  = std^2 + gamma (sigma / mu)^2                                 (score.py:389-391)
// A site reads the fields it needs; what it leaves alone is never computed (everything here inlines).
struct SdaGuide {
    float mu, sg, cx, cn, kk, var;
    bool bare;

    __device__ __forceinline__ float eps_of(float x, float net) const { return bare ? net : (x * cx) + (cn * net); }
    // x_hat = (x - sigma eps) / mu, and the likelihood cotangent (y - x_hat) / var on an observed element    (score.py:387-392)
    __device__ __forceinline__ float xhat(float x, float e) const { return (x - sg * e) / mu; }
    __device__ __forceinline__ float cot(float yv, float xh) const { return __fdiv_rn(yv - xh, var); }
    // vjp = J_eps^T ghat from J = J_net^T (cn ghat);  out = eps - sigma s,  s = ghat / mu - (sigma / mu) vjp   (score.py:394-396)
    __device__ __forceinline__ float vjp_of(float ghat, float J) const { return bare ? J : (ghat * cx) + J; }
    __device__ __forceinline__ float score(float e, float ghat, float vjp) const { return e - kk * (ghat - sg * vjp); }
    __device__ __forceinline__ float score(float e, float ghat) const { return e - kk * (ghat - 0.f); }          // (detached guidance: no vjp term)
};

// `cn` enters `bare` only: a site without one (sda_mc_finish: the VJP kernel before it has applied cn) passes 1
__device__ __forceinline__ SdaGuide sda_guide(float mu, float sg, float std = 0.f, float gamma = 0.f, float cx0 = 0.f, float cx1 = 0.f,
                                              float cn = 1.f) {
    SdaGuide g;
    g.mu = mu; g.sg = sg; g.cn = cn;
    g.bare = cx0 == 0.f && cx1 == 0.f && cn == 1.f;
    g.cx = cx0 + cx1 * sg;
    g.kk = sg / mu;
    const float rr = __fdiv_rn(sg, mu);
    g.var = __fadd_rn(__fmul_rn(std, std), __fmul_rn(gamma, __fmul_rn(rr, rr)));
    return g;
}
// from a fused launch's descriptor (sda_net1d_fuse / sda_mlp_win: the same field names)
template <class D>
__device__ __forceinline__ SdaGuide sda_guide_of(const D& f) { return sda_guide(f.coef[0], f.coef[1], f.std, f.gamma, f.cx0, f.cx1, f.cn); }

// ---- the observed lattice A = x[..., p_start:p_stop:p_step, c_start:c_stop:c_step] of a (position, channel) layout
struct SdaLatticeChan { bool on; int och; };                             // channel ch is observed, as y's column och
struct SdaLattice {
    int p_start, p_step, p_stop, c_start, c_step, c_stop, n_oc;        // n_oc: observed channels = y's row length

    // is (position ps, channel ch) observed?  and, on a hit only (a division each), its element of one image's y [positions][n_oc]
    __device__ __forceinline__ bool at(int ps, int ch) const {
        const int crel = ch - c_start, prel = ps - p_start;
        return crel >= 0 && ch < c_stop && crel % c_step == 0 && prel >= 0 && ps < p_stop && prel % p_step == 0;
    }
    __device__ __forceinline__ int y_index(int ps, int ch) const { return ((ps - p_start) / p_step) * n_oc + (ch - c_start) / c_step; }
    // the same in two halves, for a site that walks positions inside a channel: the channel half once per channel (net1d.hpp)
    __device__ __forceinline__ SdaLatticeChan channel(int ch) const {
        const int crel = ch - c_start;
        const bool on = crel >= 0 && ch < c_stop && crel % c_step == 0;
        return SdaLatticeChan{on, on ? crel / c_step : 0};
    }
    __device__ __forceinline__ bool at(const SdaLatticeChan& oc, int ps) const {
        const int prel = ps - p_start;
        return oc.on && prel >= 0 && ps < p_stop && prel % p_step == 0;
    }
    __device__ __forceinline__ int y_index(const SdaLatticeChan& oc, int ps) const { return ((ps - p_start) / p_step) * n_oc + oc.och; }
};
template <class D>
__device__ __forceinline__ SdaLattice sda_lattice_of(const D& f) {
    return SdaLattice{f.p_start, f.p_step, f.p_stop, f.c_start, f.c_step, f.c_stop, (f.c_stop - f.c_start + f.c_step - 1) / f.c_step};
}

// ---- predictor (score.py:252-253) and the tail of a fused VJP launch by `mode`
__device__ __forceinline__ float sda_pc_predict_of(float x, float out, float r, float c1) { return r * x + c1 * out; }

// 0: write out;  1: x <- r x + c1 out in place (out is not written);  2: write out and sum out^2 (the caller reduces `acc` into its
// fixed slot of `partial`: the Langevin step size stays deterministic)
struct SdaGuideTail {
    int mode;
    float r, c1;

    __device__ __forceinline__ void put(float ov, float* out, float* xs, float& acc) const {
        if (mode == 1) *xs = sda_pc_predict_of(*xs, ov, r, c1);
        else {
            *out = ov;
            acc += ov * ov;
        }
    }
};
__device__ __forceinline__ SdaGuideTail sda_guide_tail(int mode, const float* step_coef) {
    SdaGuideTail t{mode, 0.f, 0.f};
    if (mode == 1) { t.r = step_coef[0]; t.c1 = step_coef[1]; }
    return t;
}

// ---- Langevin corrector (score.py:257-261): delta = tau / mean(eps^2), x -= (delta eps + sqrt(2 delta) z) sigma
__device__ __forceinline__ void sda_langevin_step(float tot, int64_t per_sample, float tau, float& delta, float& sq) {
    delta = tau / (tot / (float)per_sample);
    sq = sqrtf(2.0f * delta);
}
__device__ __forceinline__ float sda_langevin_correct(float x, float e, float z, float delta, float sq, float sigma) {
    return x - (delta * e + sq * z) * sigma;
}
