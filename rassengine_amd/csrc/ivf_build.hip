// ivf_build.hip — the list plan of an IVF build as device code (rass_ivf_plan_lists, rass_ivf_build_device, rass_ivf_absorb;
// DESIGN.md §3 "device plan and absorb").
//
// Input: assign[n_rows] (the list of source row r) and the source's row tags (RASS_ROW_TAG_DELETED = in no list).  Output:
// exactly what the host loops of rass_ivf_build_prefix produce: list_len, list_tile0, total_tiles, slab_ids (ascending source
// row inside every list, -1 on padding) and its inverse pos_of.  A stable counting sort of the rows by list id, in two phases
// with one small host read between them in the builders (the slab is sized from total_tiles):
//
//   count   list_len by atomic adds (counts only: every position below is a function of the input) -> ONE workgroup scans
//           the nlist lengths into list_tile0, the exclusive prefix of the lengths (list_start) and the totals.
//   place   two stable 8-bit passes over the 16-bit key (a tombstoned row, or one whose id is out of range, carries 0xffff
//           and sorts behind every list).  Each pass: a 256-bin histogram per 4 096-row workgroup tile (digit-major table) ->
//           ONE workgroup scans the table in place -> every workgroup walks its tile again in 256-row chunks and ranks the
//           rows of equal digit in row order (ballots inside a wave, one LDS counter row per wave across waves).  The second
//           pass does not write a sorted array: row r at sorted index i of list l goes to slab position
//           tile0[l] * tile_rows + (i - list_start[l]).
//
// No workgroup waits on another one (no look-back, no flags): the order between the steps is the order of the launches on
// the stream, as in compact.hip.  The two table scans run on one workgroup each (0.8 M entries at 12.5 M rows): a millisecond
// next to a build that moves 50 GB.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/rass_engine.h"
#include "kernels.h"

namespace rass {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 4096;                 // rows per workgroup of the histogram and scatter launches
constexpr int kChunks = kTile / kThreads;
constexpr int kScanThreads = 1024;
constexpr int kCountLdsBins = 8192;         // list_len is privatised in LDS up to this many lists (32 KiB)
constexpr unsigned kDeadKey = 0xffffu;      // nlist <= 32768: no list has this key
constexpr int64_t kSlabLimit = 0x7fffffc0LL;

// Exclusive prefix of `v` over the workgroup's threads (thread order); *total = the workgroup's sum.  `lds`: one slot per wave.
template <int THREADS>
__device__ __forceinline__ int64_t block_exclusive(int64_t v, int64_t* lds, int64_t* total) {
    constexpr int kW = THREADS / 64;
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
    for (int w = 0; w < kW; ++w) {
        const int64_t s = lds[w];
        if (w < wave) before += s;
        all += s;
    }
    __syncthreads();   // lds is reused by the caller's next round
    *total = all;
    return before + inc - v;
}

// The sort key of source row r: its list, or kDeadKey for a row that is in no list.  *bad: a LIVE row names no list.
__device__ __forceinline__ unsigned row_key(const int32_t* __restrict__ assign, const int32_t* __restrict__ tags, int64_t r,
                                            int nlist, bool* bad) {
    *bad = false;
    if (tags[r] == RASS_ROW_TAG_DELETED) return kDeadKey;
    const int32_t l = assign[r];
    if (l < 0 || l >= nlist) {
        *bad = true;
        return kDeadKey;
    }
    return (unsigned)l;
}

// ---- count
__global__ __launch_bounds__(kThreads) void ivf_count_kernel(const int32_t* __restrict__ assign, const int32_t* __restrict__ tags,
                                                             int64_t n_rows, int nlist, int32_t* __restrict__ list_len,
                                                             int32_t* __restrict__ status) {
    __shared__ int32_t bins[kCountLdsBins];
    const bool local = nlist <= kCountLdsBins;
    if (local) {
        for (int i = threadIdx.x; i < nlist; i += kThreads) bins[i] = 0;
        __syncthreads();
    }
    bool any_bad = false;
    for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * kThreads) {
        bool bad;
        const unsigned key = row_key(assign, tags, r, nlist, &bad);
        any_bad |= bad;
        if (key == kDeadKey) continue;
        if (local) atomicAdd(&bins[key], 1);
        else atomicAdd(&list_len[key], 1);
    }
    if (any_bad) atomicOr(status, 1);
    if (local) {
        __syncthreads();
        for (int i = threadIdx.x; i < nlist; i += kThreads)
            if (bins[i]) atomicAdd(&list_len[i], bins[i]);
    }
}

// ONE workgroup: list_len[nlist] -> list_tile0 (exclusive prefix of the lists' tiles), list_start (of their lengths),
// *total_tiles, *n_live; a slab past the limit ors 2 into *status.
__global__ __launch_bounds__(kScanThreads) void ivf_list_table_kernel(const int32_t* __restrict__ list_len, int nlist,
                                                                      int tile_rows, int32_t* __restrict__ list_tile0,
                                                                      int32_t* __restrict__ list_start,
                                                                      int64_t* __restrict__ total_tiles,
                                                                      int64_t* __restrict__ n_live, int32_t* __restrict__ status) {
    __shared__ int64_t lds[kScanThreads / 64];
    const int seg = (nlist + kScanThreads - 1) / kScanThreads;
    const int a = min((int)threadIdx.x * seg, nlist), b = min(a + seg, nlist);
    int64_t tiles = 0, rows = 0;
    for (int l = a; l < b; ++l) {
        tiles += (list_len[l] + tile_rows - 1) / tile_rows;
        rows += list_len[l];
    }
    int64_t all_tiles, all_rows;
    int64_t t = block_exclusive<kScanThreads>(tiles, lds, &all_tiles);
    int64_t s = block_exclusive<kScanThreads>(rows, lds, &all_rows);
    const bool fits = all_tiles * tile_rows <= kSlabLimit;   // otherwise a tile0 may not fit its int32: nothing is placed
    for (int l = a; l < b; ++l) {
        list_tile0[l] = fits ? (int32_t)t : 0;
        list_start[l] = (int32_t)s;      // live rows <= n_rows < 2^31
        t += (list_len[l] + tile_rows - 1) / tile_rows;
        s += list_len[l];
    }
    if (threadIdx.x == 0) {
        *total_tiles = all_tiles;
        if (n_live) *n_live = all_rows;
        if (!fits) atomicOr(status, 2);
    }
}

// ---- place
// SECOND = false: the key's low digit, from assign / tags.  SECOND = true: the high digit, from the first pass's keys.
template <bool SECOND>
__device__ __forceinline__ unsigned item_key(const int32_t* __restrict__ assign, const int32_t* __restrict__ tags,
                                             const uint16_t* __restrict__ keys, int64_t i, int nlist) {
    if (SECOND) return keys[i];
    bool bad;
    return row_key(assign, tags, i, nlist, &bad);
}

template <bool SECOND>
__global__ __launch_bounds__(kThreads) void ivf_digit_hist_kernel(const int32_t* __restrict__ assign,
                                                                  const int32_t* __restrict__ tags,
                                                                  const uint16_t* __restrict__ keys, int64_t n_rows, int nlist,
                                                                  uint32_t* __restrict__ table) {
    __shared__ uint32_t bins[256];
    bins[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i0 = (int64_t)blockIdx.x * kTile;
#pragma unroll 4
    for (int c = 0; c < kChunks; ++c) {
        const int64_t i = i0 + c * kThreads + threadIdx.x;
        if (i < n_rows) {
            const unsigned key = item_key<SECOND>(assign, tags, keys, i, nlist);
            atomicAdd(&bins[SECOND ? key >> 8 : key & 255u], 1u);
        }
    }
    __syncthreads();
    table[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = bins[threadIdx.x];   // digit-major: its prefix is the sorted order
}

// ONE workgroup: table[0 .. n) -> its exclusive prefix, in place.  Every thread owns a contiguous segment.
__global__ __launch_bounds__(kScanThreads) void ivf_table_scan_kernel(uint32_t* __restrict__ table, int64_t n) {
    __shared__ int64_t lds[kScanThreads / 64];
    const int64_t seg = (n + kScanThreads - 1) / kScanThreads;
    const int64_t a = min((int64_t)threadIdx.x * seg, n), b = min(a + seg, n);
    int64_t sum = 0;
    for (int64_t i = a; i < b; ++i) sum += table[i];
    int64_t total;
    int64_t run = block_exclusive<kScanThreads>(sum, lds, &total);
    for (int64_t i = a; i < b; ++i) {
        const uint32_t c = table[i];
        table[i] = (uint32_t)run;        // < n_rows < 2^31
        run += c;
    }
}

// slab_ids[0 .. min(capacity, max(*total_tiles, 1) * tile_rows)) = -1
__global__ __launch_bounds__(kThreads) void ivf_fill_ids_kernel(int64_t* __restrict__ slab_ids, int64_t capacity,
                                                                const int64_t* __restrict__ total_tiles, int tile_rows,
                                                                const int32_t* __restrict__ status) {
    int64_t n = (*status & 2) ? 0 : max(*total_tiles, (int64_t)1) * tile_rows;
    if (n > capacity) n = capacity;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) slab_ids[i] = -1;
}

// The stable scatter of one digit.  Chunk by chunk (256 consecutive items, one per thread): the lanes of a wave that hold
// the same digit find each other with 8 ballots; the first of them leaves their number in the wave's counter row; an item's
// place is the digit's running base + the counts of the waves before its own + its rank among its wave's lanes.
template <bool SECOND>
__global__ __launch_bounds__(kThreads) void ivf_digit_scatter_kernel(
    const int32_t* __restrict__ assign, const int32_t* __restrict__ tags, const uint16_t* __restrict__ keys_in,
    const int32_t* __restrict__ rows_in, int64_t n_rows, int nlist, const uint32_t* __restrict__ table,
    uint16_t* __restrict__ keys_out, int32_t* __restrict__ rows_out,                       // first pass
    const int32_t* __restrict__ list_tile0, const int32_t* __restrict__ list_start, int tile_rows,
    int64_t* __restrict__ slab_ids, int64_t capacity, int32_t* __restrict__ pos_of, int32_t* __restrict__ status) {
    __shared__ uint32_t base[256];
    __shared__ uint32_t wave_cnt[kWaves][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    base[threadIdx.x] = table[(int64_t)threadIdx.x * gridDim.x + blockIdx.x];
#pragma unroll
    for (int w = 0; w < kWaves; ++w) wave_cnt[w][threadIdx.x] = 0;
    __syncthreads();
    const int64_t i0 = (int64_t)blockIdx.x * kTile;
    bool short_slab = false;
    for (int c = 0; c < kChunks; ++c) {
        if (i0 + c * kThreads >= n_rows) break;                 // uniform over the workgroup
        const int64_t i = i0 + c * kThreads + threadIdx.x;
        const bool valid = i < n_rows;
        const unsigned key = valid ? item_key<SECOND>(assign, tags, keys_in, i, nlist) : 0u;
        const unsigned dg = SECOND ? key >> 8 : key & 255u;
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool one = (dg >> bit) & 1u;
            const unsigned long long m = __ballot(one);
            peers &= one ? m : ~m;
        }
        const int rank = __popcll(peers & ((1ull << lane) - 1ull));
        if (valid && rank == 0) wave_cnt[wave][dg] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (valid) {
            uint32_t at = base[dg] + (uint32_t)rank;
#pragma unroll
            for (int w = 0; w < kWaves; ++w)
                if (w < wave) at += wave_cnt[w][dg];
            const int32_t row = SECOND ? rows_in[i] : (int32_t)i;
            if (!SECOND) {
                keys_out[at] = (uint16_t)key;                   // at < n_rows: the prefix count of the items sorted before
                rows_out[at] = row;
            } else if (key == kDeadKey) {
                pos_of[row] = -1;
            } else {
                const int64_t pos = (int64_t)list_tile0[key] * tile_rows + ((int64_t)at - list_start[key]);
                if (pos < capacity) {
                    slab_ids[pos] = row;
                    pos_of[row] = (int32_t)pos;                 // capacity <= the slab limit < 2^31
                } else {
                    pos_of[row] = -1;
                    short_slab = true;
                }
            }
        }
        __syncthreads();
        uint32_t add = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            add += wave_cnt[w][threadIdx.x];
            wave_cnt[w][threadIdx.x] = 0;
        }
        base[threadIdx.x] += add;
        __syncthreads();
    }
    if (SECOND && short_slab) atomicOr(status, 4);
}

// lists -> assign: one thread per slab position.  The list of tile t is the LAST list whose tile0 is <= t (the lists before
// it that share its tile0 are empty).
__global__ __launch_bounds__(kThreads) void ivf_lists_to_assign_kernel(const int32_t* __restrict__ list_tile0,
                                                                       const int32_t* __restrict__ list_len, int nlist,
                                                                       int tile_rows, const int64_t* __restrict__ slab_ids,
                                                                       int64_t slab_rows, int32_t* __restrict__ assign,
                                                                       int64_t n_assign) {
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < slab_rows; p += (int64_t)gridDim.x * kThreads) {
        const int64_t id = slab_ids[p];
        if (id < 0 || id >= n_assign) continue;
        const int32_t tile = (int32_t)(p / tile_rows);
        int lo = 0, hi = nlist;                                  // the first list whose tile0 is > tile
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (list_tile0[mid] <= tile) lo = mid + 1;
            else hi = mid;
        }
        const int l = lo - 1;
        if (l >= 0 && p - (int64_t)list_tile0[l] * tile_rows < list_len[l]) assign[id] = l;
    }
}

int64_t plan_wgs(int64_t n_rows) { return n_rows > 0 ? (n_rows + kTile - 1) / kTile : 0; }

unsigned stride_grid(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kThreads - 1) / kThreads, 2048)); }

// The caller's workspace: list_start [nlist] | digit table [256 n_wg] | first-pass keys [n_rows] | first-pass rows.
struct PlanWorkspace {
    int32_t* list_start;
    uint32_t* table;
    uint16_t* keys;
    int32_t* rows;
    size_t total;
};

PlanWorkspace plan_workspace(void* base, int64_t n_rows, int nlist) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        void* p = static_cast<unsigned char*>(base) + off;
        off = (off + bytes + 255) / 256 * 256;
        return p;
    };
    const size_t n = (size_t)std::max<int64_t>(n_rows, 1), wgs = (size_t)std::max<int64_t>(plan_wgs(n_rows), 1);
    PlanWorkspace w;
    w.list_start = static_cast<int32_t*>(take((size_t)std::max(nlist, 1) * 4));
    w.table = static_cast<uint32_t*>(take(wgs * 256 * 4));
    w.keys = static_cast<uint16_t*>(take(n * 2));
    w.rows = static_cast<int32_t*>(take(n * 4));
    w.total = off;
    return w;
}

}  // namespace

size_t ivf_plan_workspace_bytes(int64_t n_rows, int nlist) { return plan_workspace(nullptr, n_rows, nlist).total; }

hipError_t launch_ivf_plan_count(const int32_t* assign, const int32_t* tags, int64_t n_rows, int nlist, int tile_rows,
                                 int32_t* list_len, int32_t* list_tile0, int64_t* total_tiles, int64_t* n_live, int32_t* status,
                                 void* workspace, hipStream_t stream) {
    if (n_rows < 0 || n_rows > kSlabLimit || nlist < 1 || nlist > 32768 || (tile_rows != 32 && tile_rows != 64))
        return hipErrorInvalidValue;
    const PlanWorkspace w = plan_workspace(workspace, n_rows, nlist);
    hipError_t e = hipMemsetAsync(list_len, 0, (size_t)nlist * 4, stream);
    if (e == hipSuccess) e = hipMemsetAsync(status, 0, 4, stream);
    if (e != hipSuccess) return e;
    if (n_rows > 0)
        hipLaunchKernelGGL(ivf_count_kernel, dim3(std::min(stride_grid(n_rows), 512u)), dim3(kThreads), 0, stream, assign, tags,
                           n_rows, nlist, list_len, status);
    hipLaunchKernelGGL(ivf_list_table_kernel, dim3(1), dim3(kScanThreads), 0, stream, list_len, nlist, tile_rows, list_tile0,
                       w.list_start, total_tiles, n_live, status);
    return hipGetLastError();
}

hipError_t launch_ivf_plan_place(const int32_t* assign, const int32_t* tags, int64_t n_rows, int nlist, int tile_rows,
                                 const int32_t* list_tile0, const int64_t* total_tiles, int64_t* slab_ids,
                                 int64_t slab_ids_capacity, int32_t* pos_of, int32_t* status, void* workspace,
                                 hipStream_t stream) {
    if (n_rows < 0 || n_rows > kSlabLimit || nlist < 1 || nlist > 32768 || (tile_rows != 32 && tile_rows != 64) ||
        slab_ids_capacity < 0 || slab_ids_capacity > kSlabLimit)
        return hipErrorInvalidValue;
    const PlanWorkspace w = plan_workspace(workspace, n_rows, nlist);
    const unsigned wgs = (unsigned)plan_wgs(n_rows);
    hipLaunchKernelGGL(ivf_fill_ids_kernel, dim3(stride_grid(slab_ids_capacity)), dim3(kThreads), 0, stream, slab_ids,
                       slab_ids_capacity, total_tiles, tile_rows, status);
    if (wgs > 0) {
        hipLaunchKernelGGL(ivf_digit_hist_kernel<false>, dim3(wgs), dim3(kThreads), 0, stream, assign, tags,
                           (const uint16_t*)nullptr, n_rows, nlist, w.table);
        hipLaunchKernelGGL(ivf_table_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, w.table, (int64_t)wgs * 256);
        hipLaunchKernelGGL(ivf_digit_scatter_kernel<false>, dim3(wgs), dim3(kThreads), 0, stream, assign, tags,
                           (const uint16_t*)nullptr, (const int32_t*)nullptr, n_rows, nlist, (const uint32_t*)w.table, w.keys,
                           w.rows, (const int32_t*)nullptr, (const int32_t*)nullptr, tile_rows, (int64_t*)nullptr, (int64_t)0,
                           (int32_t*)nullptr, (int32_t*)nullptr);
        hipLaunchKernelGGL(ivf_digit_hist_kernel<true>, dim3(wgs), dim3(kThreads), 0, stream, (const int32_t*)nullptr,
                           (const int32_t*)nullptr, (const uint16_t*)w.keys, n_rows, nlist, w.table);
        hipLaunchKernelGGL(ivf_table_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, w.table, (int64_t)wgs * 256);
        hipLaunchKernelGGL(ivf_digit_scatter_kernel<true>, dim3(wgs), dim3(kThreads), 0, stream, (const int32_t*)nullptr,
                           (const int32_t*)nullptr, (const uint16_t*)w.keys, (const int32_t*)w.rows, n_rows, nlist,
                           (const uint32_t*)w.table, (uint16_t*)nullptr, (int32_t*)nullptr, list_tile0,
                           (const int32_t*)w.list_start, tile_rows, slab_ids, slab_ids_capacity, pos_of, status);
    }
    return hipGetLastError();
}

hipError_t launch_ivf_lists_to_assign(const int32_t* list_tile0, const int32_t* list_len, int nlist, int tile_rows,
                                      const int64_t* slab_ids, int64_t slab_rows, int32_t* assign, int64_t n_assign,
                                      hipStream_t stream) {
    if (slab_rows <= 0 || n_assign <= 0) return hipSuccess;
    hipLaunchKernelGGL(ivf_lists_to_assign_kernel, dim3(stride_grid(slab_rows)), dim3(kThreads), 0, stream, list_tile0, list_len,
                       nlist, tile_rows, slab_ids, slab_rows, assign, n_assign);
    return hipGetLastError();
}

}  // namespace rass
