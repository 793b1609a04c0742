// ivf_allow.hip — the bridge between a caller's row bitmap and an IVF probe: the allow-list scan (scan_topk.hip, ScanMode
// kAllow) tests one bitmap word per (query, 32-row tile) of the slab it streams, but a caller's bitmap names SOURCE rows and
// an IVF slab is a permutation of them (rass_ivf::d_ids, lists starting on tile boundaries, -1 on padding).  Here the
// probe plan of one launch group (plan_probe_kernel's work list) gets
//   1. its slab-order words: bit r of word (q, tile) = the caller's bit of source row d_ids[32 * tile + r], and each item's
//      query mask narrowed to the queries whose word is non-zero (ivf_allow_words_kernel);
//   2. its items compacted: those whose narrowed mask is 0 are dropped, the survivors keep their ascending tile order (the
//      insertion's tie rule needs rows in ascending order), into a second work list with its own count and the rows it
//      keeps (ivf_allow_place_kernel; block counts first, placement second, as allow.hip's plan).
// Plain vector loads, stores, ballots and atomics (LDS counters); no workgroup waits on another: two launches.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.h"

namespace rass {

namespace {

constexpr int kThreads = 256;          // = items of the work list per workgroup, in both kernels
constexpr int kHalves = kThreads / 32; // 32-lane halves: one work item each per step

// Workgroup b owns items [256 b, 256 b + 256) of the work list; a 32-lane half takes one item per step, lane r of it the
// tile's row r.  Every lane of the workgroup runs the same trip counts (n, nq and n_bitmaps are uniform), so every lane
// reaches every ballot.
__global__ __launch_bounds__(kThreads) void ivf_allow_words_kernel(const int32_t* __restrict__ work_tile,
                                                                   const int32_t* __restrict__ work_rows,
                                                                   uint32_t* __restrict__ work_mask,
                                                                   const int32_t* __restrict__ n_work, int64_t max_items,
                                                                   const int64_t* __restrict__ slab_ids,
                                                                   const uint32_t* __restrict__ allow, int64_t q_stride, int64_t words,
                                                                   int nq, uint32_t* __restrict__ slab_allow, int64_t slab_q_stride,
                                                                   int32_t* __restrict__ block_count, int64_t* __restrict__ block_rows) {
    __shared__ int sh_count;
    __shared__ int sh_rows;
    if (threadIdx.x == 0) sh_count = 0, sh_rows = 0;
    __syncthreads();
    const int64_t n = min((int64_t)*n_work, max_items);
    const int lane = threadIdx.x & 63, r = lane & 31, half = threadIdx.x >> 5;
    const int n_maps = q_stride == 0 ? 1 : nq;   // a shared bitmap: one word per tile
    for (int step = 0; step < kThreads / kHalves; ++step) {
        const int64_t i = (int64_t)blockIdx.x * kThreads + step * kHalves + half;
        const bool item = i < n;
        const int tile = item ? work_tile[i] : 0;
        const int rows = item ? work_rows[i] : 0;
        const uint32_t mask = item ? work_mask[i] : 0u;
        // the source row behind this lane's slab position: -1 on padding; past the tile's rows nothing is read
        const int64_t src = (item && r < rows) ? slab_ids[(int64_t)tile * 32 + r] : (int64_t)-1;
        const bool in_map = src >= 0 && (src >> 5) < words;
        uint32_t keep = 0;
        for (int q = 0; q < n_maps; ++q) {
            const bool wanted = q_stride == 0 ? mask != 0u : ((mask >> q) & 1u) != 0u;
            bool bit = false;
            if (wanted && in_map) bit = ((allow[(int64_t)q * q_stride + (src >> 5)] >> (src & 31)) & 1u) != 0u;
            const unsigned long long b = __ballot(bit);
            const uint32_t word = (lane & 32) ? (uint32_t)(b >> 32) : (uint32_t)b;
            // every query of a planned tile gets a defined word (the scan reads both of a wave's queries' words): 0 where the
            // item's mask does not name the query
            if (item && r == 0) slab_allow[(int64_t)q * slab_q_stride + tile] = word;
            if (word != 0u) keep |= q_stride == 0 ? mask : (1u << q);
        }
        if (item && r == 0) {
            work_mask[i] = keep;
            if (keep != 0u) {
                atomicAdd(&sh_count, 1);
                atomicAdd(&sh_rows, rows);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        block_count[blockIdx.x] = sh_count;
        block_rows[blockIdx.x] = sh_rows;
    }
}

// Workgroup b places its surviving items behind those of workgroups 0 .. b-1 (it sums their counts itself), in item order
// — the work list is ascending in tiles, so the compacted one is too.  The last workgroup writes the totals.
__global__ __launch_bounds__(kThreads) void ivf_allow_place_kernel(const int32_t* __restrict__ work_tile, const int32_t* __restrict__ work_rows,
                                                                   const uint32_t* __restrict__ work_mask,
                                                                   const int32_t* __restrict__ n_work, int64_t max_items,
                                                                   const int32_t* __restrict__ block_count,
                                                                   const int64_t* __restrict__ block_rows, int32_t* __restrict__ out_tile,
                                                                   int32_t* __restrict__ out_rows, uint32_t* __restrict__ out_mask,
                                                                   int32_t* __restrict__ out_n, int64_t* __restrict__ scanned_rows) {
    __shared__ int sh_wave[kThreads / 64];
    __shared__ long long sh_wave_rows[kThreads / 64];
    __shared__ int sh_base;
    __shared__ long long sh_base_rows;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool last = blockIdx.x == gridDim.x - 1;
    int before = 0;
    long long rows_before = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += kThreads) before += block_count[b];
    if (last)   // the rows the compacted list keeps: every workgroup's, this one's included
        for (int b = threadIdx.x; b < (int)gridDim.x; b += kThreads) rows_before += block_rows[b];
    for (int off = 32; off > 0; off >>= 1) {
        before += __shfl_xor(before, off, 64);
        rows_before += __shfl_xor(rows_before, off, 64);
    }
    if (lane == 0) sh_wave[wave] = before, sh_wave_rows[wave] = rows_before;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        long long sr = 0;
        for (int w = 0; w < kThreads / 64; ++w) s += sh_wave[w], sr += sh_wave_rows[w];
        sh_base = s;
        sh_base_rows = sr;
    }
    __syncthreads();
    const int base = sh_base;
    __syncthreads();   // sh_wave is reused below
    const int64_t n = min((int64_t)*n_work, max_items);
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint32_t m = i < n ? work_mask[i] : 0u;
    const unsigned long long b = __ballot(m != 0u);
    if (lane == 0) sh_wave[wave] = __popcll(b);
    __syncthreads();
    int pos = base + __popcll(b & ((1ull << lane) - 1ull));
    int total = 0;
    for (int w = 0; w < kThreads / 64; ++w) {
        const int c = sh_wave[w];
        if (w < wave) pos += c;
        total += c;
    }
    if (m != 0u) {   // pos < the number of surviving items <= i + 1 <= max_items: inside the lists
        out_tile[pos] = work_tile[i];
        out_rows[pos] = work_rows[i];
        out_mask[pos] = m;
    }
    if (last && threadIdx.x == 0) {
        *out_n = base + total;
        *scanned_rows = (int64_t)sh_base_rows;
    }
}

// *accum += (*add_from, where given) + the rows of the n_work first items of a work list (where given).  One workgroup.
__global__ __launch_bounds__(kThreads) void work_rows_add_kernel(const int32_t* __restrict__ work_rows, const int32_t* __restrict__ n_work,
                                                                 int64_t max_items, const int64_t* __restrict__ add_from,
                                                                 int64_t* __restrict__ accum) {
    __shared__ long long sh_wave[kThreads / 64];
    long long s = 0;
    if (work_rows != nullptr && n_work != nullptr) {
        const int64_t n = min((int64_t)*n_work, max_items);
        for (int64_t i = threadIdx.x; i < n; i += kThreads) s += work_rows[i];
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) sh_wave[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long t = add_from ? (long long)*add_from : 0;
        for (int w = 0; w < kThreads / 64; ++w) t += sh_wave[w];
        *accum += (int64_t)t;
    }
}

inline int item_blocks(int64_t max_items) { return (int)((std::max<int64_t>(max_items, 1) + kThreads - 1) / kThreads); }

}  // namespace

size_t ivf_allow_workspace_bytes(int64_t max_items) {
    return ((size_t)item_blocks(max_items) * sizeof(int64_t) + 255) / 256 * 256 + (size_t)item_blocks(max_items) * sizeof(int32_t);
}

hipError_t launch_ivf_allow_words(const int32_t* work_tile, const int32_t* work_rows, uint32_t* work_mask, const int32_t* n_work,
                                  int64_t max_items, const int64_t* slab_ids, const uint32_t* allow, int64_t q_stride, int64_t words,
                                  int nq, uint32_t* slab_allow, int64_t slab_q_stride, int32_t* out_tile, int32_t* out_rows,
                                  uint32_t* out_mask, int32_t* out_n, int64_t* scanned_rows, void* workspace, hipStream_t stream) {
    if (nq < 1 || nq > 32 || max_items < 1 || max_items > 0x7fffffc0LL / 32 || q_stride < 0 || words < 0 || slab_q_stride < 0)
        return hipErrorInvalidValue;
    if ((q_stride == 0) != (slab_q_stride == 0)) return hipErrorInvalidValue;   // a shared bitmap gives one shared slab-order bitmap
    if (slab_q_stride != 0 && slab_q_stride < max_items) return hipErrorInvalidValue;
    if (!work_tile || !work_rows || !work_mask || !n_work || !slab_ids || !allow || !slab_allow || !out_tile || !out_rows || !out_mask ||
        !out_n || !scanned_rows || !workspace)
        return hipErrorInvalidValue;
    const int blocks = item_blocks(max_items);
    int64_t* block_rows = static_cast<int64_t*>(workspace);
    int32_t* block_count =
        reinterpret_cast<int32_t*>(static_cast<unsigned char*>(workspace) + ((size_t)blocks * sizeof(int64_t) + 255) / 256 * 256);
    hipLaunchKernelGGL(ivf_allow_words_kernel, dim3(blocks), dim3(kThreads), 0, stream, work_tile, work_rows, work_mask, n_work, max_items,
                       slab_ids, allow, q_stride, words, nq, slab_allow, slab_q_stride, block_count, block_rows);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ivf_allow_place_kernel, dim3(blocks), dim3(kThreads), 0, stream, work_tile, work_rows, work_mask, n_work, max_items,
                       block_count, block_rows, out_tile, out_rows, out_mask, out_n, scanned_rows);
    return hipGetLastError();
}

hipError_t launch_work_rows_add(const int32_t* work_rows, const int32_t* n_work, int64_t max_items, const int64_t* add_from, int64_t* accum,
                                hipStream_t stream) {
    if (!accum || max_items < 0 || ((work_rows == nullptr) != (n_work == nullptr))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(work_rows_add_kernel, dim3(1), dim3(kThreads), 0, stream, work_rows, n_work, max_items, add_from, accum);
    return hipGetLastError();
}

}  // namespace rass
