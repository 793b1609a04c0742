// merge_topk.hip — K2 (second stage) and K3's post-all-gather merge of SURVEY §8a.
//
// Input: n_lists candidate lists per query, [n_lists][nq][k] (score f32, id i64; id < 0 =
// empty slot).  Output: [nq][k], best first under (score desc, id asc) — the same total
// order the scan kernel keeps, so merging per-workgroup lists, or per-GPU lists after the
// RCCL all-gather, gives exactly the single-scan result.  This is the analogue of
// OpenSearch's shard -> coordinator top-k merge (reference SHARD_COUNT, app/main.py:89).
//
// Wavefront bitonic top-k: one workgroup per query, 16 waves.  A wave pulls 64 candidates
// at a time, sorts them in registers with a 21-stage exchange network (DPP inside a row of 16 lanes, v_permlane16/32_swap
// across rows: no LDS, no barrier; round 3: 16.9 -> 13.9 us per launch against the ds_bpermute form),
// and folds them into its running best-32 with a 6-stage bitonic merge (running list in
// lanes 0..31, the new group's best 32 reversed into lanes 32..63).  The 16 per-wave lists
// meet once in LDS and wave 0 folds them the same way.  k <= 32.
//
// range_finish (below): the last step of a score-threshold search, the unsorted hits of a range scan -> the answer.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "scan_core.h"   // xor_lane

namespace rass {

constexpr int kMergeWaves = 16;
constexpr int kMergeThreads = kMergeWaves * 64;
constexpr int64_t kWorstId = 0x7fffffffffffffffLL;

struct Cand {
    float s;
    int64_t id;
};

__device__ __forceinline__ bool cand_better(const Cand& a, const Cand& b) {
    return (a.s > b.s) || (a.s == b.s && a.id < b.id);
}

template <int STRIDE>
__device__ __forceinline__ Cand xor_cand(const Cand& c, int lane) {
    Cand o;
    o.s = __int_as_float(xor_lane<STRIDE>(__float_as_int(c.s), lane));
    const int lo = xor_lane<STRIDE>((int)(c.id & 0xffffffffLL), lane);
    const int hi = xor_lane<STRIDE>((int)(c.id >> 32), lane);
    o.id = ((int64_t)hi << 32) | (uint32_t)lo;
    return o;
}

// lane (63 - lane) = lane ^ 63: across the halves, across the rows, mirrored inside the row
__device__ __forceinline__ Cand reverse_cand(const Cand& c, int lane) {
    Cand o = xor_cand<32>(c, lane);
    o = xor_cand<16>(o, lane);
    o.s = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(o.s), 0x140, 0xf, 0xf, true));
    const int lo = __builtin_amdgcn_mov_dpp((int)(o.id & 0xffffffffLL), 0x140, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp((int)(o.id >> 32), 0x140, 0xf, 0xf, true);
    o.id = ((int64_t)hi << 32) | (uint32_t)lo;
    return o;
}

// compare-exchange with lane ^ STRIDE; keep the better one when keep_better
template <int STRIDE>
__device__ __forceinline__ void cmpx(Cand& c, int lane, bool keep_better) {
    const Cand o = xor_cand<STRIDE>(c, lane);
    const bool mine_better = cand_better(c, o);
    if (mine_better != keep_better) c = o;
}

template <int SIZE, int STRIDE>
__device__ __forceinline__ void sort_steps(Cand& c, int lane) {
    if constexpr (STRIDE > 0) {
        const bool best_first = (lane & SIZE) == 0;  // SIZE == 64: always true
        const bool lower = (lane & STRIDE) == 0;
        cmpx<STRIDE>(c, lane, best_first == lower);
        sort_steps<SIZE, STRIDE / 2>(c, lane);
    }
}

// full bitonic sort of the wave's 64 candidates, best first
__device__ __forceinline__ void wave_sort64(Cand& c, int lane) {
    sort_steps<2, 1>(c, lane);
    sort_steps<4, 2>(c, lane);
    sort_steps<8, 4>(c, lane);
    sort_steps<16, 8>(c, lane);
    sort_steps<32, 16>(c, lane);
    sort_steps<64, 32>(c, lane);
}

// lanes 0..31 sorted best-first, lanes 32..63 sorted worst-first (a bitonic sequence)
// -> whole wave sorted best-first
template <int STRIDE>
__device__ __forceinline__ void merge_steps(Cand& c, int lane) {
    if constexpr (STRIDE > 0) {
        cmpx<STRIDE>(c, lane, (lane & STRIDE) == 0);
        merge_steps<STRIDE / 2>(c, lane);
    }
}
__device__ __forceinline__ void wave_bitonic_merge64(Cand& c, int lane) { merge_steps<32>(c, lane); }

// fold a sorted-best-first 64 group (only its best 32 matter) into the running list
__device__ __forceinline__ void fold_group(Cand& run, const Cand& grp_sorted, int lane) {
    // lane 32+i takes the group's element 31-i (reversed), lanes 0..31 keep the running list
    const Cand rev = reverse_cand(grp_sorted, lane);
    Cand c = (lane < 32) ? run : rev;
    wave_bitonic_merge64(c, lane);
    run = c;
}

__global__ __launch_bounds__(kMergeThreads) void merge_topk_kernel(const float* __restrict__ scores,
                                                                   const int64_t* __restrict__ ids, int n_lists,
                                                                   int /*nq = gridDim.x*/, int k, float* __restrict__ out_scores,
                                                                   int64_t* __restrict__ out_ids,
                                                                   const int64_t* __restrict__ id_map,
                                                                   int64_t score_list_stride, int64_t id_list_stride,
                                                                   MergeGroups grp, const int32_t* __restrict__ live_nq) {
    // the merge behind a scan that exited on a zero live count (the certified mode's idle fallback): its lists were never written
    if (live_nq != nullptr && __builtin_amdgcn_readfirstlane(*live_nq) == 0) return;
    __shared__ float sh_s[kMergeWaves * 32];
    __shared__ int64_t sh_i[kMergeWaves * 32];
    // Grouped form (grp.size > 0): blockIdx.x counts the queries of SEVERAL launch groups; group g's lists start
    // grp.*_stride elements after group g-1's and hold min(grp.size, nq_total - g*size) queries each.
    int q = blockIdx.x;
    if (grp.size > 0) {
        const int g = q / grp.size;
        q -= g * grp.size;
        scores += (int64_t)g * grp.score_stride;
        ids += (int64_t)g * grp.id_stride;
        out_scores += (int64_t)g * grp.out_score_stride;
        out_ids += (int64_t)g * grp.out_id_stride;
        if (grp.lists_are_dense) {  // [n_lists][nq_g][k] per group: the list stride follows the group's query count
            const int nq_g = min(grp.size, grp.nq_total - g * grp.size);
            score_list_stride = id_list_stride = (int64_t)nq_g * k;
        }
    }
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int n = n_lists * k;

    Cand run;
    run.s = -INFINITY;
    run.id = kWorstId;
    // groups of 64 consecutive candidates, dealt round-robin to the waves.  (Issuing a group's scattered loads a group ahead of
    // its sort changed nothing, 14.3 against 13.9 us per launch: with the exchanges in registers the kernel is paced by the
    // vector issue of its sixteen waves on one CU, ~1 900 instructions each.)
    for (int base = wave * 64; base < n; base += kMergeWaves * 64) {
        const int e = base + lane;
        Cand c;
        c.s = -INFINITY;
        c.id = kWorstId;
        if (e < n) {
            const int list = e / k, kk = e - list * k;
            // list strides in elements: nq*k for dense [n_lists][nq][k] arrays, larger when each
            // list is one rank's packed (scores | ids) record of the single all-gather
            const int64_t o = (int64_t)q * k + kk;
            const int64_t gi = ids[(int64_t)list * id_list_stride + o];
            const float gs = scores[(int64_t)list * score_list_stride + o];
            // NaN and -inf never rank (the scan never emits them; foreign lists might)
            if (gi >= 0 && gs > -INFINITY) {
                c.s = gs;
                c.id = gi;
            }
        }
        wave_sort64(c, lane);
        fold_group(run, c, lane);
    }
    // tree over the 16 per-wave lists (each sorted best-first in lanes 0..31): in round r the
    // waves with wave % (2<<r) == 0 fold in the list of wave + (1<<r), handed over through LDS
    Cand acc = run;
#pragma unroll 1
    for (int step = 1; step < kMergeWaves; step <<= 1) {
        const bool sender = (wave & (2 * step - 1)) == step;
        const bool receiver = (wave & (2 * step - 1)) == 0;
        if (sender && lane < 32) {
            sh_s[wave * 32 + lane] = acc.s;
            sh_i[wave * 32 + lane] = acc.id;
        }
        __syncthreads();
        if (receiver) {
            // lanes 32..63 take the partner's list reversed: lane 32+i <- element 31-i
            Cand c;
            c.s = sh_s[(wave + step) * 32 + (31 - (lane & 31))];
            c.id = sh_i[(wave + step) * 32 + (31 - (lane & 31))];
            if (lane < 32) c = acc;
            wave_bitonic_merge64(c, lane);
            acc = c;
        }
    }
    if (wave != 0) return;
    if (lane < k) {
        const bool filled = acc.id != kWorstId;
        out_scores[(int64_t)q * k + lane] = filled ? acc.s : -INFINITY;
        // id_map (IVF): candidates carry slab positions, callers get their own row ids
        out_ids[(int64_t)q * k + lane] = filled ? (id_map ? id_map[acc.id] : acc.id) : (int64_t)-1;
    }
}

hipError_t launch_merge_topk(const float* scores, const int64_t* ids, int n_lists, int nq, int k,
                             float* out_scores, int64_t* out_ids, hipStream_t stream, const int64_t* id_map,
                             int64_t score_list_stride, int64_t id_list_stride, const MergeGroups* groups,
                             const int32_t* live_nq) {
    const int64_t n = (int64_t)n_lists * k;
    if (n_lists < 1 || nq < 1 || k < 1 || k > 32 || n > kMergeMaxCandidates) return hipErrorInvalidValue;
    if (score_list_stride <= 0) score_list_stride = (int64_t)nq * k;
    if (id_list_stride <= 0) id_list_stride = (int64_t)nq * k;
    MergeGroups grp;
    if (groups) {
        grp = *groups;
        if (grp.size < 1 || grp.nq_total != nq) return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(merge_topk_kernel, dim3(nq), dim3(kMergeThreads), 0, stream, scores, ids, n_lists, nq, k,
                       out_scores, out_ids, id_map, score_list_stride, id_list_stride, grp, live_nq);
    return hipGetLastError();
}

// ---- range_finish: one workgroup per query of a range scan (scan_topk.hip kRange; kernels.h launch_range_finish).
// The emitted (score bits, row) pairs become 64-bit keys — the score's order-preserving key in the high word, 0x7fffffff - row
// in the low one, so that descending key order IS (score desc, row asc) — and are sorted by a bitonic network in LDS, padded
// with key 0 (below every real key) to the next power of two: 4 096 keys take 32 KiB.  -0.0f is keyed as +0.0f (the two compare
// equal, so the row decides); the scan's fmaf chains start from +0 and cannot produce it anyway.
constexpr int kRangeFinishThreads = 1024;

__device__ __forceinline__ unsigned range_score_key(unsigned bits) {
    if (bits == 0x80000000u) bits = 0u;
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

__global__ __launch_bounds__(kRangeFinishThreads) void range_finish_kernel(const unsigned* __restrict__ count,
                                                                             const uint2* __restrict__ hits, int cap, int64_t id_base,
                                                                             const int64_t* __restrict__ id_map,
                                                                             float* __restrict__ out_scores, int64_t* __restrict__ out_ids,
                                                                             int64_t* __restrict__ total) {
    __shared__ unsigned long long keys[kRangeMaxHits];
    const int q = blockIdx.x, tid = threadIdx.x;
    const unsigned cnt = count[q * kRangeCountStride];
    if (tid == 0) total[q] = (int64_t)cnt;
    float* os = out_scores + (int64_t)q * cap;
    int64_t* oi = out_ids + (int64_t)q * cap;
    const int n = cnt > (unsigned)cap ? 0 : (int)cnt;   // overflow: the empty list
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    const uint2* h = hits + (int64_t)q * cap;
    for (int i = tid; i < n2; i += kRangeFinishThreads) {
        unsigned long long key = 0ull;
        if (i < n) {
            const uint2 e = h[i];
            key = ((unsigned long long)range_score_key(e.x) << 32) | (unsigned long long)(0x7fffffffu - e.y);
        }
        keys[i] = key;
    }
    __syncthreads();
    for (int size = 2; size <= n2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < n2; i += kRangeFinishThreads) {
                const int j = i ^ stride;
                if (j > i) {
                    const unsigned long long a = keys[i], b = keys[j];
                    const bool descending = (i & size) == 0;
                    if ((a < b) == descending) keys[i] = b, keys[j] = a;
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < cap; i += kRangeFinishThreads) {
        float s = -INFINITY;
        int64_t id = -1;
        if (i < n) {
            const unsigned long long key = keys[i];
            const unsigned sk = (unsigned)(key >> 32);
            const int64_t row = (int64_t)(0x7fffffffu - (unsigned)key);
            s = __uint_as_float((sk & 0x80000000u) ? (sk ^ 0x80000000u) : ~sk);
            id = id_map ? id_map[row] : id_base + row;
        }
        os[i] = s;
        oi[i] = id;
    }
}

hipError_t launch_range_finish(const unsigned* count, const uint2* hits, int nq, int cap, int64_t id_base, const int64_t* id_map,
                               float* out_scores, int64_t* out_ids, int64_t* total, hipStream_t stream) {
    if (nq < 1 || cap < 1 || cap > kRangeMaxHits || !count || !hits || !out_scores || !out_ids || !total) return hipErrorInvalidValue;
    hipLaunchKernelGGL(range_finish_kernel, dim3(nq), dim3(kRangeFinishThreads), 0, stream, count, hits, cap, id_base, id_map,
                       out_scores, out_ids, total);
    return hipGetLastError();
}

}  // namespace rass
