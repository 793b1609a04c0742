// compact.hip — squeezing the tombstoned rows out of a flat index (rass_index_compact, DESIGN.md §2 "compaction").
//
// Two steps, both pure data movement (no arithmetic touches a stored value: the result is defined bit for bit):
//
//   plan    tags[n_rows] -> new_row[n_rows] (the exclusive prefix count of live rows, -1 for a tombstone), its inverse
//           src_row[n_live] and n_live.  Three launches: per-workgroup counts -> one workgroup scans the counts ->
//           scatter.  No workgroup waits on another one (no look-back, no flag): the tag array is 4 B per 4 KiB row, a
//           thousandth of the bytes moved, so a single-pass scan would buy nothing.
//   gather  a NEW slab whose block b, chunk j is written as one coalesced 1 KiB: lane L owns the 16 bytes of row
//           16 b + (L & 15), k-group L >> 4, and fetches them from the same chunk and k-group of row src_row[...] in the old
//           slab.  Runs of live rows make the reads coalesce as well; with scattered tombstones every 16-byte piece of a
//           touched source line is still consumed by this wave or the one of the neighbouring block.  Both slabs are touched
//           once: nontemporal loads and stores, as the encoder's row kernels do for their streams.
//
// tile16 (fp32, 16-column chunks) and tile16b (bf16, 32-column chunks) share the structure "16-row blocks of 1 KiB chunks in
// MFMA lane order, 16 bytes per lane": one kernel body, instantiated per element type.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/rass_engine.h"
#include "kernels.h"

namespace rass {

namespace {

constexpr int kPlanThreads = 256;
constexpr int kPlanPerThread = 8;
constexpr int kPlanTile = kPlanThreads * kPlanPerThread;   // rows per workgroup of the count and scatter launches
constexpr int kScanThreads = 1024;

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Exclusive prefix of `v` over the workgroup's threads (thread order); *total = the workgroup's sum.  `lds`: one slot per wave.
template <int THREADS>
__device__ __forceinline__ int64_t block_exclusive(int64_t v, int64_t* lds, int64_t* total) {
    constexpr int kWaves = THREADS / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int64_t up = (int64_t)__shfl_up((long long)inc, (unsigned)off, 64);
        if (lane >= off) inc += up;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    int64_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const int64_t s = lds[w];
        if (w < wave) before += s;
        all += s;
    }
    __syncthreads();   // lds is reused by the caller's next round
    *total = all;
    return before + inc - v;
}

// The live flags of this thread's kPlanPerThread consecutive rows (bit i = row r0 + i is live) and their number.
__device__ __forceinline__ unsigned live_bits(const int32_t* __restrict__ tags, int64_t r0, int64_t n_rows) {
    unsigned bits = 0;
#pragma unroll
    for (int i = 0; i < kPlanPerThread; ++i)
        if (r0 + i < n_rows && tags[r0 + i] != RASS_ROW_TAG_DELETED) bits |= 1u << i;
    return bits;
}

__global__ __launch_bounds__(kPlanThreads) void compact_count_kernel(const int32_t* __restrict__ tags, int64_t n_rows,
                                                                     int64_t* __restrict__ wg_count) {
    __shared__ int64_t lds[kPlanThreads / 64];
    const int64_t r0 = (int64_t)blockIdx.x * kPlanTile + (int64_t)threadIdx.x * kPlanPerThread;
    int64_t total;
    (void)block_exclusive<kPlanThreads>(__popc(live_bits(tags, r0, n_rows)), lds, &total);
    if (threadIdx.x == 0) wg_count[blockIdx.x] = total;
}

// ONE workgroup: wg_count[0 .. n_wg) -> its exclusive prefix, in place; *n_live = the sum.  Every thread owns a contiguous
// segment (34 entries at 70 M rows).
__global__ __launch_bounds__(kScanThreads) void compact_scan_kernel(int64_t* __restrict__ wg_count, int64_t n_wg,
                                                                    int64_t* __restrict__ n_live) {
    __shared__ int64_t lds[kScanThreads / 64];
    const int64_t seg = (n_wg + kScanThreads - 1) / kScanThreads;
    const int64_t a = (int64_t)threadIdx.x * seg, b = a + seg < n_wg ? a + seg : n_wg;
    int64_t sum = 0;
    for (int64_t i = a; i < b; ++i) sum += wg_count[i];
    int64_t total;
    int64_t run = block_exclusive<kScanThreads>(sum, lds, &total);
    for (int64_t i = a; i < b; ++i) {
        const int64_t c = wg_count[i];
        wg_count[i] = run;
        run += c;
    }
    if (threadIdx.x == 0) *n_live = total;
}

__global__ __launch_bounds__(kPlanThreads) void compact_scatter_kernel(const int32_t* __restrict__ tags, int64_t n_rows,
                                                                       const int64_t* __restrict__ wg_base,
                                                                       int64_t* __restrict__ new_row,
                                                                       int64_t* __restrict__ src_row) {
    __shared__ int64_t lds[kPlanThreads / 64];
    const int64_t r0 = (int64_t)blockIdx.x * kPlanTile + (int64_t)threadIdx.x * kPlanPerThread;
    const unsigned bits = live_bits(tags, r0, n_rows);
    int64_t total;
    int64_t at = wg_base[blockIdx.x] + block_exclusive<kPlanThreads>(__popc(bits), lds, &total);
#pragma unroll
    for (int i = 0; i < kPlanPerThread; ++i) {
        if (r0 + i >= n_rows) break;
        const bool live = (bits >> i) & 1u;
        new_row[r0 + i] = live ? at : -1;
        if (live) src_row[at++] = r0 + i;   // at < n_live <= n_rows: the prefix count of live rows below r0 + i
    }
}

// dst block b (of n_blocks), chunk j <- the pieces of rows src_row[16 b .. 16 b + 15]; rows >= n_dst (the tail of the last
// block) and rows whose source is outside [0, n_src_rows) are written as zeros.  Everything is counted in 16-byte pieces:
// a chunk is 64 of them, a block chunks_per_block * 64.  ELEM documents the instantiation (tile16: float, 16-column chunks;
// tile16b: 2-byte elements, 32-column chunks); the movement is the same.
template <class ELEM>
__global__ __launch_bounds__(256) void compact_rows_kernel(const ELEM* __restrict__ src_slab, ELEM* __restrict__ dst_slab,
                                                           int64_t row_stride, const int64_t* __restrict__ src_row,
                                                           int64_t n_dst, int64_t n_src_rows, int64_t n_blocks) {
    constexpr int kChunkCols = 256 / (int)sizeof(ELEM) / 4;   // 16 rows x kChunkCols columns = 1 KiB
    const int64_t chunks_per_block = row_stride / kChunkCols;
    const u32x4* __restrict__ src = reinterpret_cast<const u32x4*>(src_slab);
    u32x4* __restrict__ dst = reinterpret_cast<u32x4*>(dst_slab);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 15, g = lane >> 4;
    for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < n_blocks; b += (int64_t)gridDim.x * 4) {
        const int64_t row = b * 16 + m;
        const int64_t s = row < n_dst ? src_row[row] : -1;
        const bool valid = s >= 0 && s < n_src_rows;
        const u32x4* sp = src + ((valid ? s : 0) >> 4) * chunks_per_block * 64 + g * 16 + ((valid ? s : 0) & 15);
        u32x4* dp = dst + b * chunks_per_block * 64 + lane;
        // chunks_per_block is a multiple of 8 for every stride an index takes (128 n / 16, 256 n / 32): 8 loads in flight per lane
        int64_t j = 0;
        for (; j + 8 <= chunks_per_block; j += 8) {
            u32x4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = valid ? __builtin_nontemporal_load(sp + (j + u) * 64) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
            for (int u = 0; u < 8; ++u) __builtin_nontemporal_store(v[u], dp + (j + u) * 64);
        }
        for (; j < chunks_per_block; ++j) {
            const u32x4 v = valid ? __builtin_nontemporal_load(sp + j * 64) : u32x4{0u, 0u, 0u, 0u};
            __builtin_nontemporal_store(v, dp + j * 64);
        }
    }
}

template <class T>
__global__ void gather_elems_kernel(const T* __restrict__ src, T* __restrict__ dst, const int64_t* __restrict__ src_row,
                                    int64_t n, int64_t n_src) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = src_row[i];
        if (s >= 0 && s < n_src) dst[i] = src[s];
    }
}

template <class ELEM>
hipError_t launch_rows(const ELEM* src, ELEM* dst, int64_t row_stride, const int64_t* src_row, int64_t n_dst,
                       int64_t n_src_rows, hipStream_t stream) {
    const int64_t n_blocks = (n_dst + 15) / 16;
    if (n_blocks <= 0) return hipSuccess;
    int64_t grid = (n_blocks + 3) / 4;
    if (grid > 256 * 32) grid = 256 * 32;
    hipLaunchKernelGGL(compact_rows_kernel<ELEM>, dim3((unsigned)grid), dim3(256), 0, stream, src, dst, row_stride, src_row, n_dst,
                       n_src_rows, n_blocks);
    return hipGetLastError();
}

template <class T>
hipError_t launch_elems(const T* src, T* dst, const int64_t* src_row, int64_t n, int64_t n_src, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(gather_elems_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, stream, src, dst, src_row, n, n_src);
    return hipGetLastError();
}

}  // namespace

size_t compact_plan_workspace_bytes(int64_t n_rows) {
    const int64_t n_wg = n_rows > 0 ? (n_rows + kPlanTile - 1) / kPlanTile : 0;
    return (size_t)((std::max<int64_t>(n_wg, 1) * 8 + 255) / 256 * 256);
}

hipError_t launch_compact_plan(const int32_t* tags, int64_t n_rows, int64_t* new_row, int64_t* src_row, int64_t* n_live,
                               void* workspace, hipStream_t stream) {
    const int64_t n_wg = n_rows > 0 ? (n_rows + kPlanTile - 1) / kPlanTile : 0;
    if (n_wg > 0x7fffffff) return hipErrorInvalidValue;
    int64_t* wg = static_cast<int64_t*>(workspace);
    if (n_wg > 0)
        hipLaunchKernelGGL(compact_count_kernel, dim3((unsigned)n_wg), dim3(kPlanThreads), 0, stream, tags, n_rows, wg);
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, wg, n_wg, n_live);
    if (n_wg > 0)
        hipLaunchKernelGGL(compact_scatter_kernel, dim3((unsigned)n_wg), dim3(kPlanThreads), 0, stream, tags, n_rows, wg, new_row,
                           src_row);
    return hipGetLastError();
}

hipError_t launch_compact_rows_tile16(const float* src, float* dst, int64_t row_stride, const int64_t* src_row, int64_t n_dst,
                                      int64_t n_src_rows, hipStream_t stream) {
    return launch_rows<float>(src, dst, row_stride, src_row, n_dst, n_src_rows, stream);
}

hipError_t launch_compact_rows_tile16b(const void* src, void* dst, int64_t row_stride, const int64_t* src_row, int64_t n_dst,
                                       int64_t n_src_rows, hipStream_t stream) {
    return launch_rows<unsigned short>(static_cast<const unsigned short*>(src), static_cast<unsigned short*>(dst), row_stride,
                                       src_row, n_dst, n_src_rows, stream);
}

hipError_t launch_gather_i32(const int32_t* src, int32_t* dst, const int64_t* src_row, int64_t n, int64_t n_src,
                             hipStream_t stream) {
    return launch_elems<int32_t>(src, dst, src_row, n, n_src, stream);
}

hipError_t launch_gather_i64(const int64_t* src, int64_t* dst, const int64_t* src_row, int64_t n, int64_t n_src,
                             hipStream_t stream) {
    return launch_elems<int64_t>(src, dst, src_row, n, n_src, stream);
}

}  // namespace rass
