// scan_tophits.hip — the top-hits scan: per (query, group), the hits of a terms aggregation over a key column AND the top_hits
// best of those hits, in ONE corpus pass of a flat fp32 index (api_tophits.hip, rass_index_aggregate_hits_keys): OpenSearch's
// terms -> top_hits {size: n}.  The group-count scan (scan_topk.hip, kGroupCountKeys) keeps a counter and one best-row slot
// per (query, group); this one keeps the counter and the group-top scan's chain of top_hits slots (scan_core.h
// emit_group_count_top), level-major, so that count and plane 0 are byte for byte what the group-count scan leaves and both
// selects of group_topk.hip run on them unchanged, with group_hits_finish_kernel behind either.
//
// scan_tophits_f32_kernel<CH, NT> runs on scan_flat.h's loop (scan_topk_f32_kernel's flat loop restated from the blocks of
// scan_core.h), so a score is that kernel's bit for bit.  Nothing is ranked: no TopList, no sample floor, no continuation
// bound.  A (row, query) is a HIT by scan_stats.hip's rule: the row is live, passes q's plain or masked filter, has a group
// (key >= 0, row < group_key_rows), has its bit in q's bitmap where there is one, and s >= thr[q] (a NaN threshold matches
// nothing, -inf every such row; a NaN or -inf score never ranks, as in every scan).  A hit with key >= group_n sets the status
// word and is left out of every figure.
//
// The row's key travels as in scan_stats.hip: one 32-lane buffer load per tile through a descriptor of its own, requested
// AHEAD of the tile's corpus loads (tile_ahead) so that the wait that parks the tile's tags has seen it come back, and parked
// in LDS next to the tags (pair_top): no load sits inside the ranking step.  The bitmap words are wave-uniform and come by
// scalar loads through the constant address space.
//
// Plain vector loads, stores and atomics only.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "scan_flat.h"

namespace rass {

template <int NT>
struct TopHitsPolicy {
    const TopHitsArgs& a;
    float* thr;             // LDS [32]: the per-query thresholds (NaN past nq: nothing matches)
    int (*keys)[32];        // LDS [4][32]: the dumped tiles' group keys, next to their tags
    int K[2];               // the keys of the two tiles last requested
    int pair;               // 0 / 2: which two LDS images the iteration dumps into, as the loop counts it

    __device__ __forceinline__ void setup(int q, bool live) { thr[q] = live ? a.scan.range_thr[q] : __builtin_nanf(""); }
    __device__ __forceinline__ void tile_ahead(int which, const WorkItem& w) {
        K[which] = load_tile_keys(a.scan.group_keys, a.scan.group_key_rows, w);
    }
    // the tile pair's tags have just been stored: its keys, requested ahead of them, are back
    __device__ __forceinline__ void pair_top(const WorkItem&, const WorkItem&) {
        const int lane = lane_id();
        if (wave_id() == 0 && lane < 32) {
            keys[pair][lane] = K[0];
            keys[pair + 1][lane] = K[1];
        }
        pair ^= 2;
    }
    __device__ __forceinline__ void last_pair() {}
    __device__ __forceinline__ void rank(const FlatPart<NT>& c, int buf, int, int pq) {
        const ScanArgs& p = a.scan;
        const int key = keys[buf][c.r];
        const float s = c.score();
        // no group: not a hit, whatever the key's size
        bool ok = c.live() & (key >= 0) & (c.row < p.group_key_rows) & (c.q < p.nq);
        if (p.allow != nullptr) {   // a kernel argument: a scalar branch
            typedef const __attribute__((address_space(4))) unsigned* const_words;
            const const_words allow = (const_words)reinterpret_cast<uintptr_t>(p.allow);
            const int wid = wave_id();
            const int tile = __builtin_amdgcn_readfirstlane((c.row - c.r) >> 5);
            // queries past nq (zero rows, never emitted) read the last live query's word: in bounds
            const int qa = min(pq * 16 + wid, p.nq - 1), qb = min(pq * 16 + 8 + wid, p.nq - 1);
            const unsigned wa = allow[(int64_t)qa * p.allow_q_stride + tile];
            const unsigned wb = allow[(int64_t)qb * p.allow_q_stride + tile];
            ok = ok && ((((c.lane & 32) ? wb : wa) >> c.r) & 1u);
        }
        emit_group_count_top(ok && s >= thr[c.q], s, c.row, key, c.q, p.group_n, p.group_table, (unsigned)a.level_stride, a.top_hits,
                             a.count, p.group_status);
    }
};

template <int CH, int NT>
__global__ __launch_bounds__(kThreads, 2) void scan_tophits_f32_kernel(TopHitsArgs a) {
    __shared__ int sh_qfilt[32];
    __shared__ int sh_qmask[32];
    __shared__ float sh_thr[32];
    __shared__ int sh_tags[4][32];
    __shared__ int sh_keys[4][32];
    TopHitsPolicy<NT> pol{a, sh_thr, sh_keys, {0, 0}, 0};
    flat_pair_scan<CH, NT>(a.scan, FlatShared{sh_qfilt, sh_qmask, sh_tags}, pol);
}

struct TopHitsFamily {
    template <int CH, int NT>
    static constexpr auto kernel() { return &scan_tophits_f32_kernel<CH, NT>; }
};

hipError_t launch_scan_tophits_f32(const TopHitsArgs& a, int grid, hipStream_t stream) {
    const ScanArgs& s = a.scan;
    if (!flat_scan_args_ok(s, grid)) return hipErrorInvalidValue;
    if (!s.range_thr || !s.group_table || !s.group_status || !s.group_keys || !a.count) return hipErrorInvalidValue;
    if (s.group_n < 1 || s.group_n > kGroupMaxGroups || s.group_key_rows < 0 || s.group_key_rows > s.n_rows) return hipErrorInvalidValue;
    // every slot a hit lane can name lies inside the table: (top_hits - 1) planes, then (nq - 1) rows of group_n, then a key < group_n
    if (a.top_hits < 1 || a.top_hits > kGroupHitsMaxSize || (int64_t)s.group_n * a.top_hits > kGroupMaxGroups ||
        a.level_stride < (int64_t)s.nq * s.group_n || a.level_stride * a.top_hits > ((int64_t)1 << 25))   // one 32-bit slot index
        return hipErrorInvalidValue;
    if (s.allow_q_stride < 0) return hipErrorInvalidValue;
    if (s.part_scores || s.part_ids || s.q_after_score || s.q_after_id) return hipErrorInvalidValue;
    return launch_flat_family<TopHitsFamily>(a, grid, stream);
}

}  // namespace rass
