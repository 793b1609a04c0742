// group_topk.hip — the last step of a grouped (collapsed) search: the per-(query, group) maxima of a group-max scan
// (scan_topk.hip kGroupMax; kernels.h launch_group_select) -> the k best groups of every query.
//
// One workgroup per query over its n_groups slots in global memory.  A slot holds the group's best candidate key (scan_core.h
// cand_key: the score's order-preserving key in the high word, 0xffffffff - row in the low one) or 0.  The non-zero slots are
// counted: that is the query's number of groups.  No more than k of them: all are taken.  Otherwise an exact radix select over
// the 64-bit keys — eight 8-bit passes, the histogram in LDS, as cert_select_kernel (certify.hip) runs over its LDS keys, here
// with the keys re-read from the table each pass — finds the k-th largest key; rows are distinct, so keys are unique and
// exactly k slots hold a key >= it.  The taken keys meet their slot indices in LDS (4 096 x 12 bytes), a bitonic network
// sorts them as range_finish_kernel (merge_topk.hip) sorts its keys, and the rows are translated and written.
//
// The same kernel under COUNT finishes a terms aggregation (scan_topk.hip kGroupCount; kernels.h launch_group_count_select):
// the sort key of slot g is made on the fly from the slot's 32-bit counter, ((uint64)count << 32) | (0xffffffff - g), 0 for an
// empty slot — doc_count descending, then group key ascending, OpenSearch's default bucket order.  Slots are distinct, so these
// keys are unique too and the select, the gather and the sort are the ones above.  A listed bucket's score and id come from
// the slot of the group-max table the scan kept next to the counters; the counters' sum is the query's number of hits.
//
// group_stats_select_kernel finishes a stats aggregation ordered by a metric (scan_stats.hip; kernels.h launch_group_stats_select):
// the select again, its sort key made on the fly from a plane of the stats table; group_stats_gather_kernel then decodes the
// stats planes of the listed buckets.  The select's body is group_select_body.inc, included inside each select kernel.
//
// group_hits_finish_kernel runs behind the select of a grouped search with inner hits (scan_grouptop.hip; kernels.h
// launch_group_hits_finish): the table then has group_size planes, the select has read plane 0, and the finish reads every plane
// of the slots it chose.  It needs only the listed groups and the level-major table, so it also runs behind the COUNT select of
// a terms aggregation with top hits (scan_tophits.hip); where that aggregation orders its buckets by their best hit (the
// plain select over plane 0), group_counts_gather_kernel fetches the listed buckets' counters and sums a query's counters.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "scan_core.h"

namespace rass {

constexpr int kGroupSelThreads = 1024;

// hist[digit] += 1 for every lane with `on`.  The lanes sharing the first such lane's digit add their number once (the top
// bytes of a table's keys are nearly all equal: one LDS atomic per wave instead of 64 on one address), the others one each.
__device__ __forceinline__ void hist_add(unsigned* hist, bool on, unsigned digit) {
    const unsigned long long act = __ballot(on);
    if (act == 0) return;   // wave-uniform
    const int first = __builtin_amdgcn_readfirstlane(__ffsll((long long)act) - 1);
    const unsigned d0 = (unsigned)__builtin_amdgcn_readlane((int)digit, first);
    const bool same = on && digit == d0;
    const unsigned long long sm = __ballot(same);
    if (lane_id() == first) atomicAdd(&hist[d0], (unsigned)__popcll(sm));
    if (on && !same) atomicAdd(&hist[digit], 1u);
}

// What the metric order of a stats aggregation adds to the select (kernels.h launch_group_stats_select): the plane that says
// whether a slot has a value (non-zero), the plane the metric is read from, and whether the metric field is complemented.
struct MetricOrder {
    const unsigned* has;
    const unsigned* metric;
    bool flip;
};

// COUNT = false: the grouped search (counts, out_counts, total_hits unused).  COUNT = true: the terms aggregation.
template <bool COUNT>
__global__ __launch_bounds__(kGroupSelThreads) void group_select_kernel(const unsigned long long* __restrict__ table,
                                                                        const unsigned* __restrict__ counts, int n_groups, int k,
                                                                        int64_t id_base, const int64_t* __restrict__ id_map,
                                                                        float* __restrict__ out_scores, int64_t* __restrict__ out_ids,
                                                                        int32_t* __restrict__ out_groups, int64_t* __restrict__ out_counts,
                                                                        int64_t* __restrict__ total, int64_t* __restrict__ total_hits,
                                                                        const unsigned* __restrict__ status, int32_t* __restrict__ out_status) {
    constexpr bool METRIC = false;
    const MetricOrder mo{nullptr, nullptr, false};
#include "group_select_body.inc"
}

// The terms aggregation of a stats scan ordered by a metric (kernels.h launch_group_stats_select).
__global__ __launch_bounds__(kGroupSelThreads) void group_stats_select_kernel(const unsigned long long* __restrict__ table,
                                                                              const unsigned* __restrict__ counts, const MetricOrder mo,
                                                                              int n_groups, int k, int64_t id_base,
                                                                              const int64_t* __restrict__ id_map, float* __restrict__ out_scores,
                                                                              int64_t* __restrict__ out_ids, int32_t* __restrict__ out_groups,
                                                                              int64_t* __restrict__ out_counts, int64_t* __restrict__ total,
                                                                              int64_t* __restrict__ total_hits,
                                                                              const unsigned* __restrict__ status, int32_t* __restrict__ out_status) {
    constexpr bool COUNT = true, METRIC = true;
#include "group_select_body.inc"
}

// The decoded stats planes of the buckets a select listed (kernels.h launch_group_stats_gather): one thread per output cell.
__global__ void group_stats_gather_kernel(const int32_t* __restrict__ groups, const unsigned* __restrict__ vcount,
                                          const long long* __restrict__ sum, const unsigned* __restrict__ vmin,
                                          const unsigned* __restrict__ vmax, int nq, int n_groups, int size,
                                          int64_t* __restrict__ out_vcounts, int64_t* __restrict__ out_sums, int32_t* __restrict__ out_mins,
                                          int32_t* __restrict__ out_maxs) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)nq * size) return;
    const int q = (int)(i / size);
    const int g = groups[i];
    int64_t vc = 0, sm = 0;
    int32_t mn = 0, mx = 0;
    if (g >= 0 && g < n_groups) {
        const int64_t at = (int64_t)q * n_groups + g;
        vc = (int64_t)vcount[at];
        if (vc != 0) {
            sm = (int64_t)sum[at];
            mn = stats_unbias(~vmin[at]);
            mx = stats_unbias(vmax[at]);
        }
    }
    out_vcounts[i] = vc;
    out_sums[i] = sm;
    out_mins[i] = mn;
    out_maxs[i] = mx;
}

// The counters of the buckets a select over plane 0 of a top-hits table listed, and the sum of a query's counters (kernels.h
// launch_group_counts_gather): one workgroup per query.
__global__ __launch_bounds__(kGroupSelThreads) void group_counts_gather_kernel(const int32_t* __restrict__ groups,
                                                                               const unsigned* __restrict__ counts, int n_groups, int size,
                                                                               int64_t* __restrict__ out_counts,
                                                                               int64_t* __restrict__ total_hits) {
    __shared__ unsigned long long n_hits;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const unsigned* cnt = counts + (int64_t)q * n_groups;
    if (tid == 0) n_hits = 0ull;
    __syncthreads();
    unsigned long long hits = 0ull;
    for (int i = tid; i < n_groups; i += kGroupSelThreads) hits += cnt[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) hits += __shfl_xor(hits, o, 64);
    if (lane == 0 && hits) atomicAdd(&n_hits, hits);
    for (int i = tid; i < size; i += kGroupSelThreads) {
        const int g = groups[(int64_t)q * size + i];
        out_counts[(int64_t)q * size + i] = g >= 0 && g < n_groups ? (int64_t)cnt[g] : 0;
    }
    __syncthreads();
    if (tid == 0) total_hits[q] = (int64_t)n_hits;
}

// The inner hits of a group-top scan (kernels.h launch_group_hits_finish): levels 0 .. gs - 1 of every slot the select chose,
// and, where the caller asks, the capped list — those k * gs keys sorted by the bitonic network above, the k largest written.
// A row of the capped answer lies in a group whose best row ranks at least as high; were that group not among the k best
// groups, k groups would each own a better row and the row could not be in the top k: the selected groups suffice.
__global__ __launch_bounds__(kGroupSelThreads) void group_hits_finish_kernel(const unsigned long long* __restrict__ table, int nq,
                                                                             int n_groups, int k, int gs, int64_t id_base,
                                                                             const int64_t* __restrict__ id_map,
                                                                             const int32_t* __restrict__ groups, float* out_scores,
                                                                             int64_t* out_ids, float* __restrict__ cap_scores,
                                                                             int64_t* __restrict__ cap_ids,
                                                                             const unsigned* __restrict__ status,
                                                                             int32_t* __restrict__ out_status, int accumulate) {
    __shared__ unsigned long long keys[kGroupMaxK];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int64_t plane = (int64_t)nq * n_groups;
    const unsigned long long* tab = table + (int64_t)q * n_groups;
    const int32_t* grp = groups + (int64_t)q * k;
    const int n = k * gs;
    const bool capped = cap_scores != nullptr;
    if (tid == 0 && q == 0) {
        const int s = *status != 0u ? 1 : 0;
        if (!accumulate || s) *out_status = s;
    }
    auto put = [&](float* os, int64_t* oi, int64_t at, unsigned long long key) {
        float s = -INFINITY;
        int64_t id = -1;
        if (key != 0ull) {
            const int64_t row = (int64_t)(0xffffffffu - (unsigned)key);
            s = key_score((unsigned)(key >> 32));
            id = id_map ? id_map[row] : id_base + row;
        }
        os[at] = s;
        oi[at] = id;
    };
    for (int i = tid; i < n; i += kGroupSelThreads) {
        const int j = i / gs, l = i - j * gs;
        const int g = grp[j];
        const unsigned long long key = g >= 0 ? tab[(int64_t)l * plane + g] : 0ull;
        put(out_scores, out_ids, (int64_t)q * n + i, key);
        if (capped) keys[i] = key;
    }
    if (!capped) return;   // uniform over the launch
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    for (int i = n + tid; i < n2; i += kGroupSelThreads) keys[i] = 0ull;
    __syncthreads();
    for (int size = 2; size <= n2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < n2; i += kGroupSelThreads) {
                const int j = i ^ stride;
                if (j > i) {
                    const unsigned long long a = keys[i], b = keys[j];
                    const bool descending = (i & size) == 0;
                    if ((a < b) == descending) keys[i] = b, keys[j] = a;
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < k; i += kGroupSelThreads) put(cap_scores, cap_ids, (int64_t)q * k + i, i < n2 ? keys[i] : 0ull);
}

hipError_t launch_group_hits_finish(const unsigned long long* table, int nq, int n_groups, int k, int group_size, int64_t id_base,
                                    const int64_t* id_map, const int32_t* groups, float* out_scores, int64_t* out_ids,
                                    float* cap_scores, int64_t* cap_ids, const unsigned* status, int32_t* out_status, bool accumulate,
                                    hipStream_t stream) {
    if (nq < 1 || k < 1 || k > kGroupMaxK || n_groups < 1 || n_groups > kGroupMaxGroups || group_size < 1 ||
        group_size > kGroupHitsMaxSize || (int64_t)n_groups * group_size > kGroupMaxGroups || !table || !groups || !out_scores ||
        !out_ids || !status || !out_status)
        return hipErrorInvalidValue;
    if ((cap_scores == nullptr) != (cap_ids == nullptr)) return hipErrorInvalidValue;
    if (cap_scores != nullptr && (int64_t)k * group_size > kGroupMaxK) return hipErrorInvalidValue;   // the keys' 32 KiB of LDS
    hipLaunchKernelGGL(group_hits_finish_kernel, dim3(nq), dim3(kGroupSelThreads), 0, stream, table, nq, n_groups, k, group_size, id_base,
                       id_map, groups, out_scores, out_ids, cap_scores, cap_ids, status, out_status, accumulate ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_group_select(const unsigned long long* table, int nq, int n_groups, int k, int64_t id_base, const int64_t* id_map,
                               float* out_scores, int64_t* out_ids, int32_t* out_groups, int64_t* total, const unsigned* status,
                               int32_t* out_status, hipStream_t stream) {
    if (nq < 1 || k < 1 || k > kGroupMaxK || n_groups < 1 || n_groups > kGroupMaxGroups || !table || !out_scores || !out_ids ||
        !out_groups || !total || !status || !out_status)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_select_kernel<false>, dim3(nq), dim3(kGroupSelThreads), 0, stream, table, (const unsigned*)nullptr, n_groups, k,
                       id_base, id_map, out_scores, out_ids, out_groups, (int64_t*)nullptr, total, (int64_t*)nullptr, status, out_status);
    return hipGetLastError();
}

hipError_t launch_group_count_select(const unsigned* counts, const unsigned long long* best, int nq, int n_groups, int size, int64_t id_base,
                                     const int64_t* id_map, int32_t* out_groups, int64_t* out_counts, float* out_scores, int64_t* out_ids,
                                     int64_t* n_buckets, int64_t* total_hits, const unsigned* status, int32_t* out_status,
                                     hipStream_t stream) {
    if (nq < 1 || size < 1 || size > kGroupMaxK || n_groups < 1 || n_groups > kGroupMaxGroups || !counts || !best || !out_groups ||
        !out_counts || !out_scores || !out_ids || !n_buckets || !total_hits || !status || !out_status)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_select_kernel<true>, dim3(nq), dim3(kGroupSelThreads), 0, stream, best, counts, n_groups, size, id_base,
                       id_map, out_scores, out_ids, out_groups, out_counts, n_buckets, total_hits, status, out_status);
    return hipGetLastError();
}

hipError_t launch_group_stats_select(const unsigned* counts, const unsigned long long* best, const unsigned* vcount, const unsigned* vmin,
                                     const unsigned* vmax, int order_by, bool descending, int nq, int n_groups, int size, int64_t id_base,
                                     const int64_t* id_map, int32_t* out_groups, int64_t* out_counts, float* out_scores, int64_t* out_ids,
                                     int64_t* n_buckets, int64_t* total_hits, const unsigned* status, int32_t* out_status,
                                     hipStream_t stream) {
    if (order_by == kStatsByCount && descending)   // OpenSearch's default bucket order: the select as it is
        return launch_group_count_select(counts, best, nq, n_groups, size, id_base, id_map, out_groups, out_counts, out_scores, out_ids,
                                         n_buckets, total_hits, status, out_status, stream);
    if (nq < 1 || size < 1 || size > kGroupMaxK || n_groups < 1 || n_groups > kGroupMaxGroups || !counts || !best || !vcount || !vmin ||
        !vmax || !out_groups || !out_counts || !out_scores || !out_ids || !n_buckets || !total_hits || !status || !out_status)
        return hipErrorInvalidValue;
    MetricOrder mo;
    switch (order_by) {
        // the planes hold count, vcount and biased max as they order, and the biased min complemented
        case kStatsByCount: mo = MetricOrder{counts, counts, !descending}; break;
        case kStatsByValueCount: mo = MetricOrder{vcount, vcount, !descending}; break;
        case kStatsByMin: mo = MetricOrder{vcount, vmin, descending}; break;
        case kStatsByMax: mo = MetricOrder{vcount, vmax, !descending}; break;
        default: return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(group_stats_select_kernel, dim3(nq), dim3(kGroupSelThreads), 0, stream, best, counts, mo, n_groups, size, id_base,
                       id_map, out_scores, out_ids, out_groups, out_counts, n_buckets, total_hits, status, out_status);
    return hipGetLastError();
}

hipError_t launch_group_stats_gather(const int32_t* groups, const unsigned* vcount, const long long* sum, const unsigned* vmin,
                                     const unsigned* vmax, int nq, int n_groups, int size, int64_t* out_vcounts, int64_t* out_sums,
                                     int32_t* out_mins, int32_t* out_maxs, hipStream_t stream) {
    if (nq < 1 || size < 1 || size > kGroupMaxK || n_groups < 1 || n_groups > kGroupMaxGroups || !groups || !vcount || !sum || !vmin ||
        !vmax || !out_vcounts || !out_sums || !out_mins || !out_maxs)
        return hipErrorInvalidValue;
    const int64_t cells = (int64_t)nq * size;
    hipLaunchKernelGGL(group_stats_gather_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, groups, vcount, sum, vmin,
                       vmax, nq, n_groups, size, out_vcounts, out_sums, out_mins, out_maxs);
    return hipGetLastError();
}

hipError_t launch_group_counts_gather(const int32_t* groups, const unsigned* counts, int nq, int n_groups, int size,
                                      int64_t* out_counts, int64_t* total_hits, hipStream_t stream) {
    if (nq < 1 || size < 1 || size > kGroupMaxK || n_groups < 1 || n_groups > kGroupMaxGroups || !groups || !counts || !out_counts ||
        !total_hits)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_counts_gather_kernel, dim3(nq), dim3(kGroupSelThreads), 0, stream, groups, counts, n_groups, size, out_counts,
                       total_hits);
    return hipGetLastError();
}

}  // namespace rass
