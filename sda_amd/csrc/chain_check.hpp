// Argument checks the chain kernels (chain.hip) and the ensemble smoother (enks.hip) share.
#pragma once
#include "sda_common.hpp"

static inline int chain_obs_check(const sda_chain_obs* o, int d) {
    if (!o || !o->y || o->k < 1 || o->k > d || o->k > SDA_CHAIN_MAXOBS || !(o->sigma > 0.f)) return SDA_E_BADARG;
    for (int k = 0; k < o->k; ++k)
        if (o->idx[k] < 0 || o->idx[k] >= d || o->scale[k] == 0.f) return SDA_E_BADARG;
    return SDA_OK;
}
