// Linear assignment on the device: forward auction with epsilon-scaling (Bertsekas), Jacobi rounds, plus a duality-gap
// certificate computed in the same launch.  The equal-count transport LP of emd (sda/utils.py:203-219) without the host
// round trip of sda_assignment_cost (metrics.hip).
//
// One workgroup owns one problem; a launch takes a batch (grid = batch).  No workgroup ever waits for another (the rule of
// chain.hip): every hand-off inside a problem is a workgroup barrier, and problems never talk to each other.
//
// State per problem, in LDS (28 bytes per row -> n <= 4096 is 112 KiB of the 160 KiB): per column price (float64), owner
// (int32) and a best-bid slot (float64 bits + int32 row); per row col_of_row (int32).  The cost matrix stays in global memory
// (fp32, widened on load).
//
// A round: every unassigned row i scans its row against ONE price snapshot (one wave per row, lanes stride the columns,
// shuffles merge best / second), bids  p_j + (second - best) + eps  on its best column j; barrier; the highest bid of a
// column wins (ties: the lowest row), evicts the owner and becomes the price; barrier.  The resolve step takes one more
// barrier than that sentence: bids are merged with an LDS 64-bit max (prices and bids are positive doubles, which order as
// their bit patterns), then the rows that hold the maximum agree on the lowest row with an LDS min, then the winner writes.
// Rows see equal values -> lowest column; columns see equal bids -> lowest row: max and min are order independent, so the
// permutation and the prices do not depend on wave scheduling, and the host replay at the bottom of the file (SDA_HOST_EMU,
// the same __host__ __device__ functions run as loops over lanes and waves) reproduces them bit for bit.  The arithmetic of
// the auction is float64 add, subtract and compare.
//
// Work bound: a round is run only if all of its bids fit in what is left of bid_budget (every unassigned row bids in every
// round, so the count is known before the round), hence bids <= bid_budget, rounds <= bid_budget, and every other loop is
// bounded by n or by the phase cap.  An exhausted budget ends the launch with SDA_AUCTION_NOT_CONVERGED and the partial state.
//
// Latency-bound by design: one CU per problem, a round costs one row scan (n fp32 from L2 + n prices from LDS per bidder)
// and three barriers; the tail of a phase has few bidders per round.
#include "sda_common.hpp"

#include <float.h>
#include <limits.h>
#include <math.h>

#define AU_THREADS 1024
#define AU_WAVES (AU_THREADS / SDA_WAVE)
// 64-row chunks a wave can own in one round (chunk c belongs to wave c % AU_WAVES): the bid of row 64 c + l waits in lane l's
// registers between the bid step and the resolve steps
#define AU_CHUNKS ((SDA_AUCTION_MAX_N / SDA_WAVE + AU_WAVES - 1) / AU_WAVES)
#define AU_MAX_PHASES 64                // eps_rel >= 1e-12 needs 21; the cap only bounds the loop
#define AU_LDS_BYTES(n) ((size_t)28 * (size_t)(n))

// ---------------------------------------------------------------- the arithmetic, shared by the kernel and the host replay
struct au_best {
    double best, second;                // smallest and second smallest c_ij + p_j seen (equal values count twice)
    int bj;                             // lowest column index that attains `best`
};

__host__ __device__ __forceinline__ au_best au_empty() {
    au_best s;
    s.best = s.second = (double)INFINITY;
    s.bj = INT_MAX;
    return s;
}

__host__ __device__ __forceinline__ void au_see(au_best& s, double v, int j) {
    if (v < s.best || (v == s.best && j < s.bj)) { s.second = s.best; s.best = v; s.bj = j; }
    else if (v < s.second) s.second = v;
}

// summaries of two disjoint column sets -> summary of their union (commutative: both lanes of a butterfly get the same)
__host__ __device__ __forceinline__ au_best au_merge(const au_best& a, const au_best& b) {
    au_best r;
    if (b.best < a.best || (b.best == a.best && b.bj < a.bj)) {
        r.best = b.best; r.bj = b.bj; r.second = a.best < b.second ? a.best : b.second;
    } else {
        r.best = a.best; r.bj = a.bj; r.second = b.best < a.second ? b.best : a.second;
    }
    return r;
}

// what lane `lane` of the wave that scans `row` sees: 16-byte loads when every row is 16-byte aligned, dwords otherwise
template <typename P>
__host__ __device__ __forceinline__ au_best au_scan_lane(const float* __restrict__ row, int n, const P* price, int lane, bool vec) {
    au_best s = au_empty();
    if (vec) {
        for (int j = 4 * lane; j < n; j += 4 * SDA_WAVE) {
            const float4 c = *reinterpret_cast<const float4*>(row + j);
            au_see(s, (double)c.x + price[j], j);
            au_see(s, (double)c.y + price[j + 1], j + 1);
            au_see(s, (double)c.z + price[j + 2], j + 2);
            au_see(s, (double)c.w + price[j + 3], j + 3);
        }
    } else {
        for (int j = lane; j < n; j += SDA_WAVE) au_see(s, (double)row[j] + price[j], j);
    }
    return s;
}

__host__ __device__ __forceinline__ double au_bid(double pj, const au_best& s, double eps, int n) {
    const double second = n == 1 ? s.best : s.second;
    return (pj + (second - s.best)) + eps;
}

__host__ __device__ __forceinline__ bool au_outbids(double bid, int row, double slot_bid, int slot_row) {
    return bid > slot_bid || (bid == slot_bid && row < slot_row);
}

// `row` takes column j at price `bid`; returns 1 when the column was free (one row fewer is unassigned)
__host__ __device__ __forceinline__ int au_award(int j, int row, double bid, double* price, int* owner, int* col_of_row) {
    const int old = owner[j];
    if (old >= 0) col_of_row[old] = -1;
    owner[j] = row;
    price[j] = bid;
    col_of_row[row] = j;
    return old < 0;
}

__host__ __device__ __forceinline__ bool au_finite(float c) { return fabsf(c) <= FLT_MAX; }      // false for NaN, +-inf
__host__ __device__ __forceinline__ double au_eps_final(double R, double eps_rel) { return eps_rel * R; }
__host__ __device__ __forceinline__ double au_eps_first(double R, double ef) { const double e = 0.25 * R; return e > ef ? e : ef; }
__host__ __device__ __forceinline__ double au_eps_next(double eps, double ef) { const double e = 0.25 * eps; return e > ef ? e : ef; }
// certificate from the three ordered sums: dual = sum_i min_j (c_ij + p_j) - sum_j p_j is feasible for ANY prices
__host__ __device__ __forceinline__ double au_gap(double total, double sum_min, double sum_price) { return total - (sum_min - sum_price); }

static int au_check(const void* cost, int n, int batch, double eps_rel, int64_t bid_budget, const void* total, const void* gap,
                    const void* eps_final, const void* bids, const void* status, const void* col_of_row) {
    if (!cost || !total || !gap || !eps_final || !bids || !status || !col_of_row) return SDA_E_BADARG;
    if (n < 1 || batch < 1 || bid_budget < 1 || !(eps_rel >= 1e-12) || !(eps_rel <= 1.0)) return SDA_E_BADARG;
    if (reinterpret_cast<uintptr_t>(cost) & 3) return SDA_E_BADARG;
    if (n > SDA_AUCTION_MAX_N) return SDA_E_UNSUPPORTED;             // the state does not fit LDS: not served, nothing launched
    return SDA_OK;
}

#ifndef SDA_HOST_EMU
struct au_args {
    const float* cost;
    int n;
    double eps_rel;
    int64_t budget;
    double* total;
    double* gap;
    double* eps_final;
    int64_t* bids;
    int32_t* status;
    int32_t* col_of_row;
};

__device__ __forceinline__ au_best au_scan_row(const float* __restrict__ row, int n, const double* price, int lane, bool vec) {
    au_best s = au_scan_lane(row, n, price, lane, vec);
#pragma unroll
    for (int off = SDA_WAVE / 2; off > 0; off >>= 1) {
        au_best o;
        o.best = __shfl_xor(s.best, off, SDA_WAVE);
        o.second = __shfl_xor(s.second, off, SDA_WAVE);
        o.bj = __shfl_xor(s.bj, off, SDA_WAVE);
        s = au_merge(s, o);
    }
    return s;
}

// lane 0 gets v[0] + ... in the tree the host replay repeats (au_tree_host)
__device__ __forceinline__ double au_tree(double v) {
#pragma unroll
    for (int off = SDA_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, SDA_WAVE);
    return v;
}

__global__ __launch_bounds__(AU_THREADS) void auction_kernel(au_args a) {
    extern __shared__ double au_lds[];
    const int n = a.n;
    // PRICES AND BIDS ARE FLOAT64 (costs are widened on load).  In fp32 an increment of eps_final = 1e-7 R is below one ulp of
    // a price of order R: p + eps == p, a bid no longer raises the price, the same rows bid on the same columns for ever --
    // the one place this kernel could stop making progress.  In float64 eps_rel >= 1e-12 stays far above the ulp.
    double* price = au_lds;
    unsigned long long* bid_bits = reinterpret_cast<unsigned long long*>(price + n);     // best bid of the round (0 = none)
    int* owner = reinterpret_cast<int*>(bid_bits + n);
    int* bid_row = owner + n;                                                               // lowest row holding that bid
    int* col_of_row = bid_row + n;
    __shared__ double red[3 * AU_WAVES];
    __shared__ int s_unassigned, s_bad;

    const int tid = threadIdx.x, lane = tid & (SDA_WAVE - 1), wave = tid / SDA_WAVE;
    const int b = blockIdx.x;
    const int64_t nn = (int64_t)n * n;
    const float* __restrict__ cost = a.cost + (int64_t)b * nn;
    const bool vec = (n & 3) == 0 && (reinterpret_cast<uintptr_t>(cost) & 15) == 0;

    // ---- pre-pass: cmin, cmax, non-finite entries
    if (tid == 0) s_bad = 0;
    for (int j = tid; j < n; j += AU_THREADS) { price[j] = 0.0; bid_bits[j] = 0ull; bid_row[j] = INT_MAX; }
    __syncthreads();
    float lo = INFINITY, hi = -INFINITY;
    int bad = 0;
    if (vec) {
        for (int64_t e = 4 * (int64_t)tid; e < nn; e += 4 * AU_THREADS) {
            const float4 c = *reinterpret_cast<const float4*>(cost + e);
            bad |= !au_finite(c.x) | !au_finite(c.y) | !au_finite(c.z) | !au_finite(c.w);
            lo = c.x < lo ? c.x : lo; lo = c.y < lo ? c.y : lo; lo = c.z < lo ? c.z : lo; lo = c.w < lo ? c.w : lo;
            hi = c.x > hi ? c.x : hi; hi = c.y > hi ? c.y : hi; hi = c.z > hi ? c.z : hi; hi = c.w > hi ? c.w : hi;
        }
    } else {
        for (int64_t e = tid; e < nn; e += AU_THREADS) {
            const float c = cost[e];
            bad |= !au_finite(c);
            lo = c < lo ? c : lo;
            hi = c > hi ? c : hi;
        }
    }
#pragma unroll
    for (int off = SDA_WAVE / 2; off > 0; off >>= 1) {
        const float l2 = __shfl_xor(lo, off, SDA_WAVE), h2 = __shfl_xor(hi, off, SDA_WAVE);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if (bad) atomicOr(&s_bad, 1);
    if (lane == 0) { red[wave] = (double)lo; red[AU_WAVES + wave] = (double)hi; }
    __syncthreads();
    if (s_bad) {                                           // NaN / inf costs: SDA_E_BADARG, as the host solver answers
        for (int i = tid; i < n; i += AU_THREADS) a.col_of_row[(int64_t)b * n + i] = -1;
        if (tid == 0) {
            a.total[b] = (double)NAN; a.gap[b] = (double)NAN; a.eps_final[b] = 0.0; a.bids[b] = 0; a.status[b] = SDA_E_BADARG;
        }
        return;
    }
    double cmin = red[0], cmax = red[AU_WAVES];
    for (int w = 1; w < AU_WAVES; ++w) {
        cmin = red[w] < cmin ? red[w] : cmin;
        cmax = red[AU_WAVES + w] > cmax ? red[AU_WAVES + w] : cmax;
    }
    const double R = cmax - cmin;
    const double eps_final = au_eps_final(R, a.eps_rel);
    int64_t bids = 0;
    int status = SDA_AUCTION_CONVERGED;
    const int nchunks = (n + SDA_WAVE - 1) / SDA_WAVE;

    if (R == 0.0) {                                        // all costs equal: the identity is optimal, no rounds
        for (int i = tid; i < n; i += AU_THREADS) col_of_row[i] = i;
    } else {
        double eps = au_eps_first(R, eps_final);
        for (int phase = 0; phase < AU_MAX_PHASES; ++phase) {
            __syncthreads();
            for (int i = tid; i < n; i += AU_THREADS) { col_of_row[i] = -1; owner[i] = -1; }    // prices are kept
            if (tid == 0) s_unassigned = n;
            __syncthreads();
            for (;;) {                                     // rounds: at most `budget` of them (each adds >= 1 bid)
                const int un = s_unassigned;
                if (un == 0) break;
                if (bids + un > a.budget) { status = SDA_AUCTION_NOT_CONVERGED; break; }
                bids += un;
                // -- bid: every unassigned row against the same price snapshot
                int my_j[AU_CHUNKS];
                double my_bid[AU_CHUNKS];
#pragma unroll
                for (int k = 0; k < AU_CHUNKS; ++k) {
                    my_j[k] = -1;
                    my_bid[k] = 0.0;
                    const int c = wave + AU_WAVES * k;
                    if (c < nchunks) {
                        const int r = c * SDA_WAVE + lane;
                        unsigned long long mask = __ballot(r < n && col_of_row[r] < 0);
                        while (mask) {                     // <= 64 trips
                            const int l = __ffsll((long long)mask) - 1;
                            mask &= mask - 1;
                            const au_best s = au_scan_row(cost + (int64_t)(c * SDA_WAVE + l) * n, n, price, lane, vec);
                            const double bid = au_bid(price[s.bj], s, eps, n);
                            if (lane == l) { my_j[k] = s.bj; my_bid[k] = bid; }
                        }
                        if (my_j[k] >= 0) atomicMax(&bid_bits[my_j[k]], (unsigned long long)__double_as_longlong(my_bid[k]));
                    }
                }
                __syncthreads();
                // -- resolve 1: among the rows that hold a column's highest bid, the lowest row
#pragma unroll
                for (int k = 0; k < AU_CHUNKS; ++k)
                    if (my_j[k] >= 0 && bid_bits[my_j[k]] == (unsigned long long)__double_as_longlong(my_bid[k]))
                        atomicMin(&bid_row[my_j[k]], (wave + AU_WAVES * k) * SDA_WAVE + lane);
                __syncthreads();
                // -- resolve 2: the winner evicts the owner, sets the price and clears the slot (losers only look: both sides
                //    go through relaxed atomics)
#pragma unroll
                for (int k = 0; k < AU_CHUNKS; ++k) {
                    const int r = (wave + AU_WAVES * k) * SDA_WAVE + lane;
                    if (my_j[k] >= 0 && __hip_atomic_load(&bid_row[my_j[k]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == r) {
                        if (au_award(my_j[k], r, my_bid[k], price, owner, col_of_row)) atomicSub(&s_unassigned, 1);
                        bid_bits[my_j[k]] = 0ull;
                        __hip_atomic_store(&bid_row[my_j[k]], INT_MAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
                __syncthreads();
            }
            if (status != SDA_AUCTION_CONVERGED || eps <= eps_final) break;
            eps = au_eps_next(eps, eps_final);
            if (phase == AU_MAX_PHASES - 1) status = SDA_AUCTION_NOT_CONVERGED;
        }
    }
    __syncthreads();

    // ---- certificate (fixed order: wave w adds rows w, w + 16, ... in row order, then the wave totals in order)
    double total = (double)NAN, gap = (double)NAN;
    if (status == SDA_AUCTION_CONVERGED) {
        double sum_cost = 0.0, sum_min = 0.0;
        for (int i = wave; i < n; i += AU_WAVES) {
            const float* row = cost + (int64_t)i * n;
            const au_best s = au_scan_row(row, n, price, lane, vec);
            sum_cost += (double)row[col_of_row[i]];
            sum_min += s.best;
        }
        double sum_price = 0.0;
        for (int j = tid; j < n; j += AU_THREADS) sum_price += price[j];
        sum_price = au_tree(sum_price);
        if (lane == 0) { red[wave] = sum_cost; red[AU_WAVES + wave] = sum_min; red[2 * AU_WAVES + wave] = sum_price; }
        __syncthreads();
        if (tid == 0) {
            double t = 0.0, m = 0.0, p = 0.0;
            for (int w = 0; w < AU_WAVES; ++w) { t += red[w]; m += red[AU_WAVES + w]; p += red[2 * AU_WAVES + w]; }
            total = t;
            gap = au_gap(t, m, p);
        }
    }
    for (int i = tid; i < n; i += AU_THREADS) a.col_of_row[(int64_t)b * n + i] = col_of_row[i];
    if (tid == 0) {
        a.total[b] = total; a.gap[b] = gap; a.eps_final[b] = eps_final; a.bids[b] = bids; a.status[b] = status;
    }
}

extern "C" int sda_assignment_auction(const float* cost, int n, int batch, double eps_rel, int64_t bid_budget, double* total,
                                      double* gap, double* eps_final, int64_t* bids, int32_t* status, int32_t* col_of_row,
                                      void* stream) {
    const int rc = au_check(cost, n, batch, eps_rel, bid_budget, total, gap, eps_final, bids, status, col_of_row);
    if (rc != SDA_OK) return rc;
    static bool raised[SDA_MAX_DEVICES];
    const int rl = sda_raise_dyn_lds(reinterpret_cast<const void*>(auction_kernel), (int)AU_LDS_BYTES(SDA_AUCTION_MAX_N), raised);
    if (rl != SDA_OK) return rl;
    au_args a;
    a.cost = cost; a.n = n; a.eps_rel = eps_rel;
    a.budget = bid_budget < (int64_t)1 << 62 ? bid_budget : (int64_t)1 << 62;
    a.total = total; a.gap = gap; a.eps_final = eps_final; a.bids = bids; a.status = status; a.col_of_row = col_of_row;
    hipLaunchKernelGGL(auction_kernel, dim3((unsigned)batch), dim3(AU_THREADS), AU_LDS_BYTES(n), (hipStream_t)stream, a);
    return sda_launch_status();
}

#else  // SDA_HOST_EMU
// ---------------------------------------------------------------- CPU replay (tests only; libsda_emu.so): the same
// __host__ __device__ functions, lanes and waves as loops over HOST arrays.  Where the device merges lanes with shuffles the
// replay runs the same butterfly over an array of 64 lane states; where it resolves bids with an LDS max and min the replay
// takes the bidders one by one through au_outbids (the same order-independent winner).
#include <vector>

static au_best au_scan_row_host(const float* row, int n, const double* price, bool vec) {
    au_best s[SDA_WAVE], t[SDA_WAVE];
    for (int lane = 0; lane < SDA_WAVE; ++lane) s[lane] = au_scan_lane(row, n, price, lane, vec);
    for (int off = SDA_WAVE / 2; off > 0; off >>= 1) {
        for (int lane = 0; lane < SDA_WAVE; ++lane) t[lane] = au_merge(s[lane], s[lane ^ off]);
        for (int lane = 0; lane < SDA_WAVE; ++lane) s[lane] = t[lane];
    }
    return s[0];
}

static double au_tree_host(double* v) {                    // lane 0 of the device's shuffle-down tree
    for (int off = SDA_WAVE / 2; off > 0; off >>= 1)
        for (int lane = 0; lane < off; ++lane) v[lane] += v[lane + off];
    return v[0];
}

static void au_solve_host(const float* cost, int n, double eps_rel, int64_t budget, double* total_out, double* gap_out,
                          double* eps_out, int64_t* bids_out, int32_t* status_out, int32_t* cor_out) {
    const int64_t nn = (int64_t)n * n;
    const bool vec = (n & 3) == 0 && (reinterpret_cast<uintptr_t>(cost) & 15) == 0;
    float lo = INFINITY, hi = -INFINITY;
    bool bad = false;
    for (int64_t e = 0; e < nn; ++e) {
        const float c = cost[e];
        bad |= !au_finite(c);
        lo = c < lo ? c : lo;
        hi = c > hi ? c : hi;
    }
    if (bad) {
        for (int i = 0; i < n; ++i) cor_out[i] = -1;
        *total_out = (double)NAN; *gap_out = (double)NAN; *eps_out = 0.0; *bids_out = 0; *status_out = SDA_E_BADARG;
        return;
    }
    std::vector<double> price(n, 0.0), slot_bid(n, 0.0), my_bid(n);
    std::vector<int> owner(n, -1), slot_row(n, INT_MAX), col_of_row(n, -1), my_j(n);
    const double R = (double)hi - (double)lo;
    const double eps_final = au_eps_final(R, eps_rel);
    int64_t bids = 0;
    int status = SDA_AUCTION_CONVERGED;
    const int nchunks = (n + SDA_WAVE - 1) / SDA_WAVE;
    if (R == 0.0) {
        for (int i = 0; i < n; ++i) col_of_row[i] = i;
    } else {
        double eps = au_eps_first(R, eps_final);
        for (int phase = 0; phase < AU_MAX_PHASES; ++phase) {
            for (int i = 0; i < n; ++i) { col_of_row[i] = -1; owner[i] = -1; }
            int unassigned = n;
            for (;;) {
                const int un = unassigned;
                if (un == 0) break;
                if (bids + un > budget) { status = SDA_AUCTION_NOT_CONVERGED; break; }
                bids += un;
                for (int i = 0; i < n; ++i) my_j[i] = -1;
                for (int wave = 0; wave < AU_WAVES; ++wave)
                    for (int k = 0; k < AU_CHUNKS; ++k) {
                        const int c = wave + AU_WAVES * k;
                        if (c >= nchunks) continue;
                        for (int l = 0; l < SDA_WAVE; ++l) {
                            const int r = c * SDA_WAVE + l;
                            if (r >= n || col_of_row[r] >= 0) continue;
                            const au_best s = au_scan_row_host(cost + (int64_t)r * n, n, price.data(), vec);
                            my_j[r] = s.bj;
                            my_bid[r] = au_bid(price[s.bj], s, eps, n);
                        }
                    }
                for (int r = 0; r < n; ++r)
                    if (my_j[r] >= 0 && au_outbids(my_bid[r], r, slot_bid[my_j[r]], slot_row[my_j[r]])) {
                        slot_bid[my_j[r]] = my_bid[r];
                        slot_row[my_j[r]] = r;
                    }
                for (int r = 0; r < n; ++r)
                    if (my_j[r] >= 0 && slot_row[my_j[r]] == r)
                        unassigned -= au_award(my_j[r], r, my_bid[r], price.data(), owner.data(), col_of_row.data());
                for (int r = 0; r < n; ++r)
                    if (my_j[r] >= 0) { slot_bid[my_j[r]] = 0.0; slot_row[my_j[r]] = INT_MAX; }
            }
            if (status != SDA_AUCTION_CONVERGED || eps <= eps_final) break;
            eps = au_eps_next(eps, eps_final);
            if (phase == AU_MAX_PHASES - 1) status = SDA_AUCTION_NOT_CONVERGED;
        }
    }
    double total = (double)NAN, gap = (double)NAN;
    if (status == SDA_AUCTION_CONVERGED) {
        double t = 0.0, m = 0.0, p = 0.0;
        std::vector<double> part(AU_THREADS, 0.0);
        for (int tid = 0; tid < AU_THREADS; ++tid)
            for (int j = tid; j < n; j += AU_THREADS) part[tid] += price[j];
        for (int wave = 0; wave < AU_WAVES; ++wave) {
            double sum_cost = 0.0, sum_min = 0.0;
            for (int i = wave; i < n; i += AU_WAVES) {
                const float* row = cost + (int64_t)i * n;
                const au_best s = au_scan_row_host(row, n, price.data(), vec);
                sum_cost += (double)row[col_of_row[i]];
                sum_min += s.best;
            }
            t += sum_cost;
            m += sum_min;
            p += au_tree_host(part.data() + wave * SDA_WAVE);
        }
        total = t;
        gap = au_gap(t, m, p);
    }
    for (int i = 0; i < n; ++i) cor_out[i] = col_of_row[i];
    *total_out = total; *gap_out = gap; *eps_out = eps_final; *bids_out = bids; *status_out = status;
}

extern "C" int sda_assignment_auction_host(const float* cost, int n, int batch, double eps_rel, int64_t bid_budget, double* total,
                                           double* gap, double* eps_final, int64_t* bids, int32_t* status, int32_t* col_of_row) {
    const int rc = au_check(cost, n, batch, eps_rel, bid_budget, total, gap, eps_final, bids, status, col_of_row);
    if (rc != SDA_OK) return rc;
    const int64_t budget = bid_budget < (int64_t)1 << 62 ? bid_budget : (int64_t)1 << 62;
    for (int b = 0; b < batch; ++b)
        au_solve_host(cost + (int64_t)b * n * n, n, eps_rel, budget, total + b, gap + b, eps_final + b, bids + b, status + b,
                      col_of_row + (int64_t)b * n);
    return SDA_OK;
}
#endif  // SDA_HOST_EMU
