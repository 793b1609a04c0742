// scan_stats.hip — the stats scan: per (query, group), the hits of a terms aggregation over a key column AND the count, sum,
// min and max of an int32 value column over those hits, in ONE corpus pass of a flat fp32 index (api_stats.hip,
// rass_index_aggregate_stats_keys): OpenSearch's stats / min / max / sum / avg / value_count sub-aggregations.
//
// scan_stats_f32_kernel<CH, NT> runs on scan_flat.h's loop (scan_topk_f32_kernel's flat loop restated from the blocks of
// scan_core.h), so a score is that kernel's bit for bit.  Nothing is ranked: no TopList, no sample floor, no continuation
// bound.  A (row, query) is a HIT when the row is live, passes q's plain or masked filter, has a group (key >= 0, row <
// group_key_rows), has its bit in q's bitmap where there is one, and s >= thr[q] (kRange's rule: a NaN threshold matches
// nothing, -inf every such row; a NaN or -inf score never ranks, as in every scan).  A hit with key >= group_n sets the status
// word and is left out.  All arithmetic on the values is integer: the table is a function of the input alone.
//
// The row's key and value travel as the keys do in scan_grouptop.hip: each one 32-lane buffer load per tile through a
// descriptor of its own, requested AHEAD of the tile's corpus loads (tile_ahead) so that the wait that parks the tile's tags
// has seen them come back, and parked in LDS next to the tags (pair_top): no load sits inside the ranking step.  A NULL key
// column (one group: every key 0) and a value column that was never set (every value kStatsMissing) get a descriptor of zero
// records: the load stays in the instruction stream — straight-line code keeps hipcc's vmcnt counts exact, as for the tags — but
// returns 0 without a memory request, and the value's constant is substituted under a scalar select.  The bitmap words are
// wave-uniform and come by scalar loads through the constant address space, as in scan_grouptop.hip.
//
// Plain vector loads, stores and atomics only.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "scan_flat.h"

namespace rass {

// max over the 32 lanes of my half of the wave (xor strides 1 .. 16 stay inside a half), in registers
__device__ __forceinline__ unsigned half_max_u32(unsigned v, int lane) {
    v = max(v, (unsigned)xor_lane<1>((int)v, lane));
    v = max(v, (unsigned)xor_lane<2>((int)v, lane));
    v = max(v, (unsigned)xor_lane<4>((int)v, lane));
    v = max(v, (unsigned)xor_lane<8>((int)v, lane));
    v = max(v, (unsigned)xor_lane<16>((int)v, lane));
    return v;
}
template <int STRIDE>
__device__ __forceinline__ unsigned long long xor_lane_u64(unsigned long long v, int lane) {
    const unsigned lo = (unsigned)xor_lane<STRIDE>((int)(unsigned)v, lane), hi = (unsigned)xor_lane<STRIDE>((int)(unsigned)(v >> 32), lane);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long half_max_u64(unsigned long long v, int lane) {
    v = max(v, xor_lane_u64<1>(v, lane));
    v = max(v, xor_lane_u64<2>(v, lane));
    v = max(v, xor_lane_u64<4>(v, lane));
    v = max(v, xor_lane_u64<8>(v, lane));
    v = max(v, xor_lane_u64<16>(v, lane));
    return v;
}
__device__ __forceinline__ long long half_sum_i64(long long v, int lane) {
    v += (long long)xor_lane_u64<1>((unsigned long long)v, lane);
    v += (long long)xor_lane_u64<2>((unsigned long long)v, lane);
    v += (long long)xor_lane_u64<4>((unsigned long long)v, lane);
    v += (long long)xor_lane_u64<8>((unsigned long long)v, lane);
    v += (long long)xor_lane_u64<16>((unsigned long long)v, lane);
    return v;
}

// The emission of a stats scan, in the place of insert_candidates: emit_group_count (scan_core.h) with four more planes.  A
// half-wave holds one query's 32 rows of a tile; `hit` says which count, g is the row's group (>= 0), val its value.  Slot of a
// hit: q * n_groups + g of every plane (one 32-bit index < 2^25 from wave-uniform bases), all zeroed by the caller.
// Nothing happens under a scalar branch where the wave has no hit.  A document's chunks are adjacent rows, so the hits of a half
// usually share one group: where every hit lane of a half agrees with the half's first hit lane (ballot, readlane) the REDUCED
// path folds the half's hits in registers — count and vcount as popcounts of ballots, sum, min, max and the best key over
// DPP / permlane exchanges — and the first hit lane alone issues the atomics: at most six per (tile, query), and with a NULL
// key column, where every hit of a query meets in ONE slot, that is what keeps the scan usable.  Otherwise, the PER-LANE
// path, every hit lane issues its own.  Integer add and max commute and associate: either path leaves the same table.
// vmax, vmin and best keep emit_group_max's relaxed pre-read and issue the atomic only where it raises the slot; a slot only
// grows, so a stale read costs a redundant atomic, never a lost one.  A hit without a value touches count and best only.
struct StatsPlanes {
    unsigned long long* best;
    unsigned* count;
    unsigned* vcount;
    long long* sum;
    unsigned* vmin;
    unsigned* vmax;
};
__device__ __forceinline__ void emit_group_stats(bool hit, float s, int row, int g, int val, int q, int n_groups, const StatsPlanes& t,
                                                 unsigned* status) {
    const bool inside = (unsigned)g < (unsigned)n_groups;
    hit = hit && s > -INFINITY;   // NaN and -inf never rank: no hit, no status
    if (hit && !inside) __hip_atomic_store(status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    hit = hit && inside;
    const unsigned long long b = __ballot(hit);
    if (b == 0) return;   // wave-uniform
    const unsigned lo = (unsigned)b, hi = (unsigned)(b >> 32);
    // the first hit lane of each half (a half without hits: any lane of it, nothing is compared with its key)
    const int f_lo = __builtin_amdgcn_readfirstlane(lo ? __builtin_ctz(lo) : 0);
    const int f_hi = __builtin_amdgcn_readfirstlane(hi ? 32 + __builtin_ctz(hi) : 32);
    const unsigned g_lo = (unsigned)__builtin_amdgcn_readlane(g, f_lo), g_hi = (unsigned)__builtin_amdgcn_readlane(g, f_hi);
    const int lane = lane_id();
    const bool upper = (lane & 32) != 0;
    const unsigned long long d = __ballot(hit && (unsigned)g != (upper ? g_hi : g_lo));
    const bool shared_lo = (unsigned)d == 0u, shared_hi = (unsigned)(d >> 32) == 0u;
    const bool shared = upper ? shared_hi : shared_lo;   // my half's hits are of one group
    const bool has = hit && val != kStatsMissing;
    const unsigned long long hb = __ballot(has);
    // this lane's own contribution; 0 is every fold's identity
    unsigned c = hit ? 1u : 0u, vc = has ? 1u : 0u;
    long long sm = has ? (long long)val : 0ll;
    unsigned mx = has ? stats_bias(val) : 0u, mn = has ? ~stats_bias(val) : 0u;
    unsigned long long key = hit ? cand_key(s, row) : 0ull;
    // the reduced path, where a half with more than one hit shares a group (wave-uniform)
    if ((shared_lo && (lo & (lo - 1u)) != 0u) || (shared_hi && (hi & (hi - 1u)) != 0u)) {
        const long long rsm = half_sum_i64(sm, lane);
        const unsigned rmx = half_max_u32(mx, lane), rmn = half_max_u32(mn, lane);
        const unsigned long long rkey = half_max_u64(key, lane);
        if (shared) {
            c = (unsigned)__popc(upper ? hi : lo);
            vc = (unsigned)__popc(upper ? (unsigned)(hb >> 32) : (unsigned)hb);
            sm = rsm, mx = rmx, mn = rmn, key = rkey;
            // the half's first hit lane issues for all of them; a half WITHOUT a hit has none (f_lo / f_hi then name a lane
            // that is no hit, whose group may be anything: it must stay out)
            hit = hit && lane == (upper ? f_hi : f_lo);
        }
    }
    if (!hit) return;
    const unsigned slot = (unsigned)q * (unsigned)n_groups + (unsigned)g;
    atomicAdd(t.count + slot, c);
    if (vc != 0u) {
        atomicAdd(t.vcount + slot, vc);
        if (sm != 0ll) atomicAdd(reinterpret_cast<unsigned long long*>(t.sum) + slot, (unsigned long long)sm);   // two's complement
        if (mx > __hip_atomic_load(t.vmax + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(t.vmax + slot, mx);
        if (mn > __hip_atomic_load(t.vmin + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(t.vmin + slot, mn);
    }
    if (key > __hip_atomic_load(t.best + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(t.best + slot, key);
}

// One int32 word per row of a tile (its key, its value), one per lane & 31 as load_tag: a descriptor of its own over the tile's
// rows that have the word — none where the column is nullptr, for a run-ahead tile past the end, or at or past `col_rows`:
// zero records, 0 comes back and no memory request is made.
__device__ __forceinline__ int load_tile_words(const int32_t* __restrict__ col, int col_rows, const WorkItem& w) {
    const int left = col_rows - w.tile * kTileRows;
    const int n = col == nullptr ? 0 : (left < w.rows ? (left < 0 ? 0 : left) : w.rows);
    const __amdgpu_buffer_rsrc_t d = make_rsrc(reinterpret_cast<uint64_t>(col + (int64_t)w.tile * kTileRows), (unsigned)(n * 4));
    return (int)__builtin_amdgcn_raw_buffer_load_b32(d, (lane_id() & 31) * 4, 0, 0);
}

template <int NT>
struct StatsPolicy {
    const StatsArgs& a;
    float* thr;             // LDS [32]: the per-query thresholds (NaN past nq: nothing matches)
    int (*keys)[32];        // LDS [4][32]: the dumped tiles' group keys and values, next to their tags
    int (*vals)[32];
    int K[2], V[2];         // the words of the two tiles last requested
    int pair;               // 0 / 2: which two LDS images the iteration dumps into, as the loop counts it

    __device__ __forceinline__ void setup(int q, bool live) { thr[q] = live ? a.scan.range_thr[q] : __builtin_nanf(""); }
    __device__ __forceinline__ void tile_ahead(int which, const WorkItem& w) {
        K[which] = load_tile_words(a.scan.group_keys, a.scan.group_key_rows, w);
        V[which] = load_tile_words(a.values, a.scan.n_rows, w);
    }
    // the tile pair's tags have just been stored: its keys and values, requested ahead of them, are back
    __device__ __forceinline__ void pair_top(const WorkItem&, const WorkItem&) {
        const int lane = lane_id();
        if (wave_id() == 0 && lane < 32) {
            keys[pair][lane] = K[0];
            keys[pair + 1][lane] = K[1];
            vals[pair][lane] = V[0];
            vals[pair + 1][lane] = V[1];
        }
        pair ^= 2;
    }
    __device__ __forceinline__ void last_pair() {}
    __device__ __forceinline__ void rank(const FlatPart<NT>& c, int buf, int, int pq) {
        const ScanArgs& p = a.scan;
        const int key = keys[buf][c.r];
        const int raw = vals[buf][c.r];
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
        const int val = a.values != nullptr ? raw : kStatsMissing;   // a column never set: a scalar select
        emit_group_stats(ok && s >= thr[c.q], s, c.row, key, val, c.q, p.group_n,
                         StatsPlanes{p.group_table, a.count, a.vcount, a.sum, a.vmin, a.vmax}, p.group_status);
    }
};

template <int CH, int NT>
__global__ __launch_bounds__(kThreads, 2) void scan_stats_f32_kernel(StatsArgs a) {
    __shared__ int sh_qfilt[32];
    __shared__ int sh_qmask[32];
    __shared__ float sh_thr[32];
    __shared__ int sh_tags[4][32];
    __shared__ int sh_keys[4][32];
    __shared__ int sh_vals[4][32];
    StatsPolicy<NT> pol{a, sh_thr, sh_keys, sh_vals, {0, 0}, {0, 0}, 0};
    flat_pair_scan<CH, NT>(a.scan, FlatShared{sh_qfilt, sh_qmask, sh_tags}, pol);
}

struct StatsFamily {
    template <int CH, int NT>
    static constexpr auto kernel() { return &scan_stats_f32_kernel<CH, NT>; }
};

hipError_t launch_scan_stats_f32(const StatsArgs& a, int grid, hipStream_t stream) {
    const ScanArgs& s = a.scan;
    if (!flat_scan_args_ok(s, grid)) return hipErrorInvalidValue;
    if (!s.range_thr || !s.group_table || !s.group_status || !a.count || !a.vcount || !a.sum || !a.vmin || !a.vmax) return hipErrorInvalidValue;
    // every slot a hit lane can name lies inside the planes: (nq - 1) rows of group_n, then a key < group_n
    if (s.group_n < 1 || s.group_n > kGroupMaxGroups || s.group_key_rows < 0 || s.group_key_rows > s.n_rows) return hipErrorInvalidValue;
    if (s.group_keys == nullptr && s.group_n != 1) return hipErrorInvalidValue;
    if (s.allow_q_stride < 0) return hipErrorInvalidValue;
    if (s.part_scores || s.part_ids || s.q_after_score || s.q_after_id) return hipErrorInvalidValue;
    return launch_flat_family<StatsFamily>(a, grid, stream);
}

}  // namespace rass
