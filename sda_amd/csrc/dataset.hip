// The device-resident trajectory dataset (sda/utils.py:58-86 TrajectoryDataset behind a shuffled DataLoader; sda_amd/data.py): one launch
// gathers a whole shuffled, randomly windowed batch from data [N][L][F] (N trajectories of L frames of F values) into out [rows][W F].
// The host route runs one randint, one narrow and one flatten per ITEM, collates and uploads; here both draws are keyed -- like the loss
// noise of train_loss.hip -- on (seed, global batch index s), and s may live in device memory, so the gather replays as the first node of a
// captured training step.
//   spe = ceil(N / batch) batches per epoch;  epoch e = s / spe, batch i = s % spe of it, row b of the batch is position p = i batch + b
//   trajectory  n_b     = perm_e(p): a four-round balanced Feistel network on the 2h-bit words, 4^h the smallest power of four >= N, with
//                         cycle walking (apply again while the result is >= N: the restriction of a permutation of [0, 4^h) to the cycle
//                         structure over [0, N) is a permutation of [0, N); 4^h < 4 N bounds the expected walk by 4).  Round r maps
//                         (l, r) -> (r, l ^ (w & (2^h - 1))), w = word 0 of Philox at the `shuffle` counter of philox.hpp.  Stateless, O(1)
//                         per row: no sort, no table, nothing kept between launches.
//   first frame start_b = (u (L - W + 1)) >> 32 in [0, L - W], u = word 0 of Philox at the `window` counter, the product in 64 bits.
//   out[b][.]           = the W F contiguous floats from ((n_b L) + start_b) F on.
// One workgroup per chunk of WB_CHUNK = 1024 elements of one row.  Its (n_b, start_b) depend on blockIdx and the arguments alone: every
// wave forms them once, uniformly.  A 16-byte path (one quad per thread) where F % 4 == 0 and data / out are 16-byte aligned -- every window
// then starts on a 16-byte boundary --, otherwise a scalar path in which thread t copies elements t, t + 256, t + 512, t + 768 of the chunk
// (64 consecutive dwords per wave and instruction).  Plain vector loads and stores, one writer per element, 64-bit element offsets, no LDS,
// no atomics.  A row whose position lies past the epoch's end (p >= N: a captured full-batch launch replayed at the epoch's short last
// batch) is left unwritten: nothing is read or written out of bounds whatever the device counter holds.
#include "sda_common.hpp"

#include "philox.hpp"

#define WB_THREADS 256
#define WB_CHUNK 1024            // elements of a row per workgroup

static inline bool wb_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// h: 4^h is the smallest power of four >= N (N < 2^31: h <= 16)
__host__ __device__ __forceinline__ int wb_half_bits(int64_t N) {
    int h = 0;
    while (((int64_t)1 << (2 * h)) < N) ++h;
    return h;
}

// perm_e(p), p in [0, N)
__host__ __device__ __forceinline__ int64_t wb_perm(int64_t p, int64_t N, int h, int64_t e, uint32_t k0, uint32_t k1) {
    const uint32_t mask = (1u << h) - 1u;
    uint64_t x = (uint64_t)p;
    do {
        uint32_t l = (uint32_t)(x >> h), r = (uint32_t)x & mask;
        for (int rd = 0; rd < 4; ++rd) {
            const uint32_t t = l ^ (philox_shuffle_word(rd, r, e, k0, k1) & mask);
            l = r;
            r = t;
        }
        x = ((uint64_t)l << h) | r;
    } while (x >= (uint64_t)N);
    return (int64_t)x;
}

// (n_b, start_b) of row b of global batch s; false where the row lies past the epoch's end
__host__ __device__ __forceinline__ bool wb_index(int64_t N, int64_t L, int64_t W, int64_t batch, int64_t spe, int h, uint32_t k0,
                                                  uint32_t k1, int64_t s, int64_t b, int64_t& n, int64_t& start) {
    const int64_t e = s / spe, p = (s - e * spe) * batch + b;
    if (s < 0 || p >= N) return false;
    n = wb_perm(p, N, h, e, k0, k1);
    start = (int64_t)(((uint64_t)philox_window_word((uint32_t)b, s, k0, k1) * (uint64_t)(L - W + 1)) >> 32);
    return true;
}

__global__ __launch_bounds__(WB_THREADS) void window_batch_kernel(const float* __restrict__ data, int64_t N, int64_t L, int64_t F,
                                                                  int64_t W, int64_t batch, int64_t spe, int h, int chunks, uint32_t k0,
                                                                  uint32_t k1, int64_t step, const int64_t* __restrict__ step_dev,
                                                                  int vec, float* __restrict__ out) {
    if (step_dev) step = step_dev[0];
    const int b = (int)(blockIdx.x / (unsigned)chunks);                 // (the grid holds exactly rows * chunks workgroups: b < rows)
    const int64_t c0 = (int64_t)(blockIdx.x - (unsigned)b * (unsigned)chunks) * WB_CHUNK;
    int64_t n, start;
    if (!wb_index(N, L, W, batch, spe, h, k0, k1, step, b, n, start)) return;
    const int64_t per_row = W * F;
    const float* __restrict__ src = data + (n * L + start) * F;
    float* __restrict__ dst = out + (int64_t)b * per_row;
    if (vec) {
        const int64_t e = c0 + 4 * (int64_t)threadIdx.x;                 // (per_row % 4 == 0: the quad is whole)
        if (e < per_row) *reinterpret_cast<float4*>(dst + e) = *reinterpret_cast<const float4*>(src + e);
    } else {
#pragma unroll
        for (int j = 0; j < WB_CHUNK / WB_THREADS; ++j) {
            const int64_t e = c0 + j * WB_THREADS + threadIdx.x;
            if (e < per_row) dst[e] = src[e];
        }
    }
}

// the checks both entries share (F = 1 for the plan); by_value: also the by-value step's batch must lie inside its epoch
static int wb_check(int64_t N, int64_t L, int64_t F, int64_t W, int64_t batch, int64_t rows, int64_t step, bool by_value) {
    if (N < 1 || L < 1 || F < 1 || W < 1 || batch < 1 || W > L || rows < 1 || rows > batch || step < 0) return SDA_E_BADARG;
    if (N > 0x7fffffffLL || L > 0x7fffffffLL || batch > 0x7fffffffLL) return SDA_E_UNSUPPORTED;
    if (by_value) {
        const int64_t spe = (N + batch - 1) / batch;
        if ((step % spe) * batch + rows > N) return SDA_E_BADARG;
    }
    // rows * ceil(W F / 1024) workgroups fit the grid, and N L F elements an int64 offset
    if (F > (0x7fffffffLL * WB_CHUNK) / W || F > INT64_MAX / (N * L)) return SDA_E_UNSUPPORTED;
    if (((W * F + WB_CHUNK - 1) / WB_CHUNK) * rows > 0x7fffffffLL) return SDA_E_UNSUPPORTED;
    return SDA_OK;
}

extern "C" int sda_window_batch(const float* data, int64_t N, int64_t L, int64_t F, int64_t W, int64_t batch, int64_t rows, uint64_t seed,
                                int64_t step, const int64_t* step_dev, float* out, void* stream) {
    if (!data || !out) return SDA_E_BADARG;
    const int rc = wb_check(N, L, F, W, batch, rows, step, step_dev == nullptr);
    if (rc != SDA_OK) return rc;
    const int64_t chunks = (W * F + WB_CHUNK - 1) / WB_CHUNK;
    const int vec = (F & 3) == 0 && wb_aligned16(data) && wb_aligned16(out);
    hipLaunchKernelGGL(window_batch_kernel, dim3((unsigned)(chunks * rows)), dim3(WB_THREADS), 0, (hipStream_t)stream, data, N, L, F, W,
                       batch, (N + batch - 1) / batch, wb_half_bits(N), (int)chunks, (uint32_t)seed, (uint32_t)(seed >> 32), step, step_dev,
                       vec, out);
    return sda_launch_status();
}

extern "C" int sda_window_batch_plan(int64_t N, int64_t L, int64_t W, int64_t batch, uint64_t seed, int64_t step, int64_t rows,
                                     int64_t* src_row, int64_t* start) {
    if (!src_row || !start) return SDA_E_BADARG;
    const int rc = wb_check(N, L, 1, W, batch, rows, step, true);
    if (rc != SDA_OK) return rc;
    const int64_t spe = (N + batch - 1) / batch;
    const int h = wb_half_bits(N);
    for (int64_t b = 0; b < rows; ++b)
        if (!wb_index(N, L, W, batch, spe, h, (uint32_t)seed, (uint32_t)(seed >> 32), step, b, src_row[b], start[b])) return SDA_E_BADARG;
    return SDA_OK;
}
