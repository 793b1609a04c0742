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
// group_hits_finish_kernel runs behind the select of a grouped search with inner hits (scan_grouptop.hip; kernels.h
// launch_group_hits_finish): the table then has group_size planes, the select has read plane 0, and the finish reads every plane
// of the slots it chose.
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

// COUNT = false: the grouped search (counts, out_counts, total_hits unused).  COUNT = true: the terms aggregation.
template <bool COUNT>
__global__ __launch_bounds__(kGroupSelThreads) void group_select_kernel(const unsigned long long* __restrict__ table,
                                                                        const unsigned* __restrict__ counts, int n_groups, int k,
                                                                        int64_t id_base, const int64_t* __restrict__ id_map,
                                                                        float* __restrict__ out_scores, int64_t* __restrict__ out_ids,
                                                                        int32_t* __restrict__ out_groups, int64_t* __restrict__ out_counts,
                                                                        int64_t* __restrict__ total, int64_t* __restrict__ total_hits,
                                                                        const unsigned* __restrict__ status, int32_t* __restrict__ out_status) {
    __shared__ unsigned long long keys[kGroupMaxK];
    __shared__ int grp[kGroupMaxK];
    __shared__ unsigned hist[256];
    __shared__ int sh_digit, sh_rank, n_sel, n_live;
    __shared__ unsigned long long n_hits;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const unsigned long long* tab = table + (int64_t)q * n_groups;
    const unsigned* cnt = COUNT ? counts + (int64_t)q * n_groups : nullptr;
    // the sort key of slot i: the group's best candidate key, or (count, 0xffffffff - i); 0 = an empty slot
    auto key_of = [&](int i) -> unsigned long long {
        if (!COUNT) return tab[i];
        const unsigned c = cnt[i];
        return c != 0u ? ((unsigned long long)c << 32) | (unsigned long long)(0xffffffffu - (unsigned)i) : 0ull;
    };
    if (tid == 0) {
        n_sel = 0;
        n_live = 0;
        n_hits = 0ull;
    }
    __syncthreads();
    int mine = 0;
    unsigned long long hits = 0ull;
    for (int i = tid; i < n_groups; i += kGroupSelThreads) {
        if (COUNT) {
            const unsigned c = cnt[i];
            mine += c != 0u ? 1 : 0;
            hits += c;
        } else {
            mine += tab[i] != 0ull ? 1 : 0;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if (lane == 0 && mine) atomicAdd(&n_live, mine);
    if (COUNT) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) hits += __shfl_xor(hits, o, 64);
        if (lane == 0 && hits) atomicAdd(&n_hits, hits);
    }
    __syncthreads();
    const int live = n_live;
    if (tid == 0) total[q] = (int64_t)live;
    if (COUNT && tid == 0) total_hits[q] = (int64_t)n_hits;
    if (tid == 0 && q == 0) *out_status = *status != 0u ? 1 : 0;   // the scan's out-of-range flag, handed to the caller

    // T: the k-th largest key where more than k slots are taken (selected = keys >= T), else 1 (every non-zero slot)
    unsigned long long T = 1ull;
    if (live > k) {
        unsigned long long prefix = 0, pmask = 0;
        int rank = k;
        for (int shift = 56; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0u;
            __syncthreads();
            // whole rounds of the workgroup: hist_add's ballots need every lane of a wave in the same iteration
            for (int i0 = 0; i0 < n_groups; i0 += kGroupSelThreads) {
                const int i = i0 + tid;
                const unsigned long long key = i < n_groups ? key_of(i) : 0ull;
                hist_add(hist, key != 0ull && (key & pmask) == prefix, (unsigned)(key >> shift) & 255u);
            }
            __syncthreads();
            if (wid == 0) {   // lane l: digits 4l .. 4l+3; the largest digit d with #(digit >= d) >= rank
                const unsigned c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
                const unsigned own = c0 + c1 + c2 + c3;
                unsigned suf = own;   // inclusive suffix over lanes >= l
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const unsigned v = __shfl_down(suf, o, 64);
                    if (lane + o < 64) suf += v;
                }
                const unsigned above = suf - own;
                const unsigned s3 = above + c3, s2 = s3 + c2, s1 = s2 + c1, s0 = s1 + c0;
                const unsigned r = (unsigned)rank;
                int d = -1;
                unsigned sup = 0;   // #(digit > d)
                if (s0 >= r) { d = 4 * lane; sup = s1; }
                if (s1 >= r) { d = 4 * lane + 1; sup = s2; }
                if (s2 >= r) { d = 4 * lane + 2; sup = s3; }
                if (s3 >= r) { d = 4 * lane + 3; sup = above; }
                const unsigned long long b = __ballot(d >= 0);
                const int top = 63 - __clzll(b);
                if (lane == top) {
                    sh_digit = d;
                    sh_rank = rank - (int)sup;
                }
            }
            __syncthreads();
            prefix |= (unsigned long long)sh_digit << shift;
            pmask |= 255ull << shift;
            rank = sh_rank;
            __syncthreads();
        }
        T = prefix;
    }
    // gather the taken keys with their slots (min(live, k) of them), pad to a power of two with key 0, sort descending
    const int n = live < k ? live : k;
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    for (int i = tid; i < n_groups; i += kGroupSelThreads) {
        const unsigned long long key = key_of(i);
        if (key >= T) {
            const int pos = atomicAdd(&n_sel, 1);
            if (pos < kGroupMaxK) {
                keys[pos] = key;
                grp[pos] = i;
            }
        }
    }
    for (int i = n + tid; i < n2; i += kGroupSelThreads) keys[i] = 0ull;   // [n, n2): no gathered key lands there
    __syncthreads();
    for (int size = 2; size <= n2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < n2; i += kGroupSelThreads) {
                const int j = i ^ stride;
                if (j > i) {
                    const unsigned long long a = keys[i], b = keys[j];
                    const bool descending = (i & size) == 0;
                    if ((a < b) == descending) {
                        keys[i] = b, keys[j] = a;
                        const int ga = grp[i];
                        grp[i] = grp[j], grp[j] = ga;
                    }
                }
            }
            __syncthreads();
        }
    float* os = out_scores + (int64_t)q * k;
    int64_t* oi = out_ids + (int64_t)q * k;
    int32_t* og = out_groups + (int64_t)q * k;
    for (int i = tid; i < k; i += kGroupSelThreads) {
        float s = -INFINITY;
        int64_t id = -1, c = 0;
        int32_t g = -1;
        if (i < n) {
            g = grp[i];
            c = COUNT ? (int64_t)(keys[i] >> 32) : 0;
            const unsigned long long key = COUNT ? tab[g] : keys[i];   // the bucket's best row: a counted slot has one
            const int64_t row = (int64_t)(0xffffffffu - (unsigned)key);
            s = key_score((unsigned)(key >> 32));
            id = id_map ? id_map[row] : id_base + row;
        }
        os[i] = s;
        oi[i] = id;
        og[i] = g;
        if (COUNT) out_counts[(int64_t)q * k + i] = c;
    }
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

}  // namespace rass
