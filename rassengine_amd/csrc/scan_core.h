// scan_core.h — device-side building blocks shared by the kernels that stream a tile16 fp32 slab through
// v_mfma_f32_16x16x4_f32 with the K axis split over 8 waves: the fused scan + top-k (scan_topk.hip) and the
// k-means assignment of the IVF build (kmeans.hip).  The pieces that do not depend on the element type — buffer
// resources (make_rsrc), the lane exchange (xor_lane) and the half-wave lists — also serve the bf16 / int8 scans
// (scan_bf16.hip, scan_i8.hip) and the merge (merge_topk.hip).  Not part of any ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rass {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kWaves = 8;
constexpr int kThreads = kWaves * 64;
constexpr int kTileRows = 32;
constexpr int kPitch = 36;  // floats per query row of the LDS partial image (32 rows + pad)

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// One tile's A fragments for one wave: 2 M-tiles x CH chunks of 16 B per lane.
template <int CH>
struct TileRegs {
    f32x4 a[2][CH];
    int tag;
};

// Wave-uniform buffer descriptors of one tile: corpus rows and row tags.  The range check
// drops every lane past the end (rows beyond n_rows, or a whole run-ahead tile past the last
// one): zeros come back and no memory request is made.
struct TileDesc {
    __amdgpu_buffer_rsrc_t rows;
    __amdgpu_buffer_rsrc_t tags;
};

// One unit of work of a workgroup: a 32-row slab tile, how many of its rows exist, and which
// queries of the batch may rank its rows (all of them for the flat scan; for IVF the queries
// that probe the list the tile belongs to).
struct WorkItem {
    int tile;
    int rows;
    unsigned mask;
};

// Which work a workgroup iterates over: every tile of one slab (flat), the tiles of a device-built probe plan
// over one slab (IVF), or the tiles of SEVERAL slabs — one per index of a cross-index query batch — each item
// naming its own slab and tag array (MULTI: concurrent users' per-user indices share one launch).
// kFlatSample is kFlat under its own kernel name: the sample pass that finds the score floors (ScanArgs::floors),
// kept apart so that per-kernel profiles do not average the short sample launches into the scan's.
// kFlatGroups: ONE launch scans the same slab for several launch groups of <= 32 queries (ScanArgs::wgs_per_group
// workgroups each): the coarse stage of an IVF batch (4 096 centroids for 1 024 queries in one launch instead of 32).
// kIvfGroups: ONE launch walks the probe plans of several launch groups (each its own work list, item count, queries and
// lists): the fine stage of an IVF batch without a launch boundary — ramp-up, tail, gap — between the groups.
// kFlatSampleGroups: the sample passes of several launch groups in one launch (a batch call's 32 passes of 20 us each).
// kRange: a flat scan that RANKS nothing: every row scoring >= the query's threshold is counted and emitted unsorted
// (emit_range below; ScanArgs::range_*), for the score-threshold search.  No sample pass, no floor, no TopList.
// kGroupMax: a flat scan that ranks nothing either: every matching row is folded into the running maximum of its (query,
// group) slot (emit_group_max below; ScanArgs::group_*), for the grouped (collapsed) search.  No sample pass, no floor, no TopList.
// kAllow: the top-k scan within a per-query row bitmap (ScanArgs::allow), under its own kernel name.  It walks a work list
// as kIvf does — the tiles in which some query of the launch group has a bit set (allow.hip builds it) — and a row ranks for
// query q only where bit (row & 31) of q's word of the tile is set.  No sample pass and no floor: a floor is only valid under
// the predicate it was sampled with.
// kGroupCount: kRange's hits, emitted as kGroupMax emits: every row scoring >= the query's threshold adds 1 to the counter of
// its (query, group) slot and is folded into the slot's running maximum (emit_group_count below; ScanArgs::count_table with
// group_* and range_thr), for the terms aggregation.  No sample pass, no floor, no TopList.
// kGroupMaxKeys / kGroupCountKeys: kGroupMax / kGroupCount with the row's group taken from a KEY COLUMN (ScanArgs::group_keys,
// one int32 per row: >= 0 the group, < 0 no group) instead of a bit field of its tag, and, where ScanArgs::allow is set, within
// a row bitmap as kAllow tests it.  The tag still decides tombstones and the per-query filters.  The key travels as the tag
// does: one 32-lane buffer load per tile through a descriptor of its own (load_tile_keys below), parked in LDS for the ranking
// step.  Still a flat scan: every tile is streamed whatever the bitmap holds.
enum ScanMode { kFlat = 0, kIvf = 1, kMulti = 2, kFlatSample = 3, kFlatGroups = 4, kIvfGroups = 5, kFlatSampleGroups = 6, kRange = 7,
                kGroupMax = 8, kAllow = 9, kGroupCount = 10, kGroupMaxKeys = 11, kGroupCountKeys = 12 };
constexpr bool mode_has_keys(int mode) { return mode == kGroupMaxKeys || mode == kGroupCountKeys; }
constexpr bool mode_is_flat(int mode) {
    return mode == kFlat || mode == kFlatSample || mode == kFlatGroups || mode == kFlatSampleGroups || mode == kRange ||
           mode == kGroupMax || mode == kGroupCount || mode_has_keys(mode);
}
constexpr bool mode_is_sample(int mode) { return mode == kFlatSample || mode == kFlatSampleGroups; }

// A raw buffer resource of `bytes` records at `addr`.  The descriptor must be PROVABLY wave-uniform or hipcc wraps every
// buffer op in a waterfall loop: pin its inputs with readfirstlane (guide T20).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(uint64_t addr, unsigned bytes) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)addr), hi = __builtin_amdgcn_readfirstlane((uint32_t)(addr >> 32));
    const unsigned nb = __builtin_amdgcn_readfirstlane(bytes);
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), /*stride*/ 0, (int)nb, 0x00020000);
}

__device__ __forceinline__ TileDesc make_tile_desc(const float* __restrict__ X, int64_t row_stride,
                                                   const int32_t* __restrict__ row_tag, const WorkItem& w) {
    const int rows_here = w.rows;
    const int64_t base_row = (int64_t)w.tile * kTileRows;
    // The descriptor must be PROVABLY wave-uniform or hipcc wraps every buffer op in a
    // waterfall loop: pin its inputs with readfirstlane (guide T20).
    const uint64_t base_u = reinterpret_cast<uint64_t>(X + base_row * row_stride);
    const uint32_t base_lo = __builtin_amdgcn_readfirstlane((uint32_t)base_u);
    const uint32_t base_hi = __builtin_amdgcn_readfirstlane((uint32_t)(base_u >> 32));
    const unsigned blocks_here = (unsigned)(rows_here + 15) >> 4;  // tile16: whole 16-row blocks
    const unsigned bytes = __builtin_amdgcn_readfirstlane(blocks_here * 16u * (unsigned)row_stride * 4u);
    TileDesc d;
    d.rows = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<float*>(((uint64_t)base_hi << 32) | base_lo),
                                               /*stride*/ 0, (int)bytes, 0x00020000);
    // Row tags: always loaded (straight-line code keeps hipcc's vmcnt counts exact); with no
    // tag array the descriptor has zero records: the load returns 0 and costs no traffic.
    const bool has_tags = row_tag != nullptr;
    const uint64_t tbase_u = has_tags ? reinterpret_cast<uint64_t>(row_tag + base_row) : base_u;
    const uint32_t tlo = __builtin_amdgcn_readfirstlane((uint32_t)tbase_u);
    const uint32_t thi = __builtin_amdgcn_readfirstlane((uint32_t)(tbase_u >> 32));
    const unsigned tbytes = __builtin_amdgcn_readfirstlane(has_tags ? (unsigned)(rows_here * 4) : 0u);
    d.tags = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<int32_t*>(((uint64_t)thi << 32) | tlo), 0,
                                               (int)tbytes, 0x00020000);
    return d;
}

// voff: this lane's byte offset inside a chunk (ONE VGPR for every load of the kernel); soff: the wave-uniform
// part (M-tile and chunk), which goes into the instruction's SGPR / immediate offset fields.  Folding it into
// per-load VGPR offsets, as the first version did, cost ~10 VGPRs the main loop does not have.
__device__ __forceinline__ f32x4 load_chunk(const TileDesc& d, int voff, int soff) {
#ifndef RASS_SCAN_AUX      // cache policy of the corpus stream: 2 = nt (read once); the micro-benchmarks sweep it (-DRASS_SCAN_AUX=<bits>)
#define RASS_SCAN_AUX 2
#endif
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(d.rows, voff, soff, RASS_SCAN_AUX));
}

__device__ __forceinline__ int load_tag(const TileDesc& d) {
    return (int)__builtin_amdgcn_raw_buffer_load_b32(d.tags, (lane_id() & 31) * 4, 0, 0);
}

// The group keys of a tile's 32 rows (kGroupMaxKeys / kGroupCountKeys), one per lane & 31 as load_tag: a descriptor of its
// own over the tile's rows that have a key (none for a run-ahead tile past the end: zero records, no traffic).  A lane past
// the records reads 0; the ranking step drops such a row by its number, not by what it read.
__device__ __forceinline__ int load_tile_keys(const int32_t* __restrict__ keys, int key_rows, const WorkItem& w) {
    const int left = key_rows - w.tile * kTileRows;
    const int n = left < w.rows ? (left < 0 ? 0 : left) : w.rows;
    const __amdgpu_buffer_rsrc_t d = make_rsrc(reinterpret_cast<uint64_t>(keys + (int64_t)w.tile * kTileRows), (unsigned)(n * 4));
    return (int)__builtin_amdgcn_raw_buffer_load_b32(d, (lane_id() & 31) * 4, 0, 0);
}

// Prologue: all of a tile's loads, in the order multiply_and_refill consumes them.  `soff0`: byte offset of the K
// panel these registers hold (0 unless the wave's K slice is walked in two panels: the wide-row kernel, dim > 1024).
template <int CH, bool TAGS = true>
__device__ __forceinline__ void issue_tile_loads(TileRegs<CH>& r, const TileDesc& d, int voff_lane, int mt_step,
                                                 int soff0 = 0) {
    if (TAGS) r.tag = load_tag(d);
#pragma unroll
    for (int j = 0; j < CH; ++j)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) r.a[mt][j] = load_chunk(d, voff_lane, soff0 + mt * mt_step + j * 1024);
}

// Multiply the resident tile and, chunk by chunk, re-issue each consumed register's load
// for the tile two steps ahead (`next`): about two tiles (32 KiB per wave, 256 KiB per CU)
// stay in flight at all times instead of one tile requested in a burst after the previous
// one has fully arrived.  sched_barrier(0) per chunk pins the load placement (hipcc would
// otherwise sink the loads behind the whole MFMA block).
//
// `between(j)` runs after chunk j's MFMAs were issued: the ranking of the PREVIOUS tile pair is cut into
// parts and placed there, so its VALU / LDS / scalar work issues while this wave's (and its SIMD partner's)
// MFMAs execute on the matrix pipe (a v_mfma_f32_16x16x4_f32 occupies the pipe for 32 cycles but takes only a
// few to issue).  Ranked in a phase of its own behind the barrier — as the first version did — it left the
// matrix pipe idle while all 8 waves ranked in lockstep: 72 us of a 690 us launch at B = 32.
//
// ZERO = false continues the accumulators of the previous call (the second K panel of a wide row: the fmaf chain of a
// wave's slice runs on in k order); `soff0` is the panel's byte offset for the refill loads.
template <int CH, int NT, bool TAGS = true, bool ZERO = true, typename Between>
__device__ __forceinline__ void multiply_and_refill(TileRegs<CH>& r, const f32x4 (&qf)[NT][CH],
                                                    f32x4 (&acc)[2][NT], const TileDesc& next, int voff_lane,
                                                    int mt_step, Between&& between, int soff0 = 0) {
    if (ZERO) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (TAGS) r.tag = load_tag(next);  // the k-means kernel streams centroids: no row tags
#pragma unroll
    for (int j = 0; j < CH; ++j) {
        // The 2 x NT accumulators are advanced ROUND-ROBIN, one k-step at a time: a dependent
        // v_mfma_f32_16x16x4_f32 can issue 40 cycles after its producer but the pipe takes a new one every 32, so
        // back-to-back MFMAs on one accumulator (what hipcc emitted for the second M-tile when left to itself:
        // two chains of four) leave the pipe idle 20 % of the time whenever the SIMD's other wave is not in its
        // MFMA phase.  With >= 2 independent accumulators between a producer and its consumer there is no bubble.
        const f32x4 a0 = r.a[0][j], a1 = r.a[1][j];
#define RASS_KSTEP(comp)                                                                                              \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) {                                                               \
        acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.comp, qf[nt][j].comp, acc[0][nt], 0, 0, 0);              \
        acc[1][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.comp, qf[nt][j].comp, acc[1][nt], 0, 0, 0);              \
    }
        RASS_KSTEP(x)
        RASS_KSTEP(y)
        RASS_KSTEP(z)
        RASS_KSTEP(w)
#undef RASS_KSTEP
        r.a[0][j] = load_chunk(next, voff_lane, soff0 + j * 1024);
        r.a[1][j] = load_chunk(next, voff_lane, soff0 + mt_step + j * 1024);
        __builtin_amdgcn_sched_barrier(0);
        between(j);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ---- the 64-query pair kernel's half-tile blocks (scan_topk.hip, scan_topk_f32_pair_kernel) ---------------------------------
// One 16-row block (half a tile) of A fragments for one wave: CH chunks of 16 B per lane.  The pair kernel multiplies a tile
// as two such blocks, each against 4 N-tiles of queries, where TileRegs / multiply_and_refill multiply two blocks against 2.
template <int CH>
struct HalfRegs {
    f32x4 a[CH];
};

// `soff0`: byte offset of the block inside its tile (0, or mt_step for the second block).  The sched_barrier per load keeps
// the prologue's loads in the order the main loop re-issues them: hipcc reorders them otherwise, and its s_waitcnt counts in
// the loop — merged over the loop entry and the back edge — then wait for nearly every load in flight at the first chunks
// of every iteration (vmcnt(3) of 17 where vmcnt(16) serves).
template <int CH>
__device__ __forceinline__ void issue_half_loads(HalfRegs<CH>& r, const TileDesc& d, int voff_lane, int soff0) {
#pragma unroll
    for (int j = 0; j < CH; ++j) {
        r.a[j] = load_chunk(d, voff_lane, soff0 + j * 1024);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// multiply_and_refill for one block: the same k-ordered v_mfma_f32_16x16x4_f32 chain per (row, query) from zero — so the same
// partial, bit for bit — with the NT accumulators advanced round-robin (NT - 1 >= 2 independent MFMAs between a producer and
// its consumer), each consumed register re-loaded from the same block of the `next` tile, before(j) ahead of chunk j's MFMAs
// and between(j) after them.  before(j) is where the ranking ISSUES its LDS reads (pinned there by a sched_barrier: hipcc sinks
// them to their first use otherwise); between(j) consumes them, 16 MFMAs (>= 512 pipe cycles) later, so they have landed when
// the ranking asks for them.  That sched_barrier holds back LDS instructions and MFMAs only (mask 0x16: VALU, SALU and VMEM may
// cross): a full one also pins the caller's loop-top work — next tile's descriptor, tag load — ahead of chunk 0's first MFMA,
// where hipcc otherwise threads it between the MFMAs, and that cost the stripped pass 7-10 us of 1 050.
template <int CH, int NT, typename Before, typename Between>
__device__ __forceinline__ void multiply_and_refill_half(HalfRegs<CH>& r, const f32x4 (&qf)[NT][CH], f32x4 (&acc)[NT],
                                                         const TileDesc& next, int voff_lane, int soff0,
                                                         Before&& before, Between&& between) {
    static_assert(NT >= 3, "a dependent MFMA issues 40 cycles after its producer: keep two others between them");
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < CH; ++j) {
        before(j);
        __builtin_amdgcn_sched_barrier(0x16);
        const f32x4 a0 = r.a[j];
#define RASS_KSTEP(comp)                                                                                              \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt)                                                                 \
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.comp, qf[nt][j].comp, acc[nt], 0, 0, 0);
        RASS_KSTEP(x)
        RASS_KSTEP(y)
        RASS_KSTEP(z)
        RASS_KSTEP(w)
#undef RASS_KSTEP
        r.a[j] = load_chunk(next, voff_lane, soff0 + j * 1024);
        __builtin_amdgcn_sched_barrier(0);
        between(j);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// Order-preserving u32 key of a finite float score (larger score <-> larger key; every finite score's key is
// >= 0x00800000, so 0 can stand for "no score"): the sample floor's selection counts keys by ballot.
__device__ __forceinline__ unsigned score_key(float s) {
    const unsigned u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_score(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// The sample floor's radix selection (scan_topk.hip, scan_bf16.hip, scan_i8.hip) runs over the top kFloorBits bits of the
// order-preserving keys: the truncation only LOWERS the floor, by < 2^-11 of its value.
constexpr int kFloorBits = 20;

// The emission of a range scan (kRange), in the place of insert_candidates: a half-wave holds one query's 32 rows of a tile.
// One ballot; where a half has hits, its first lane adds their number to the query's counter (one vector atomic per (tile,
// query) at the most) and every hitting lane stores (score bits, local row) at counter + its rank among the half's hits while
// that is below `cap`.  The counter runs on past cap: it is the exact total.  Which workgroup lands where depends on timing;
// range_finish sorts the pairs under a total order, so the answer does not.
__device__ __forceinline__ void emit_range(bool hit, float s, int row, unsigned* count, uint2* hits, int cap) {
    hit = hit && s > -INFINITY;   // NaN and -inf never rank (include/rass_engine.h, "Scores that are not finite")
    const unsigned long long b = __ballot(hit);
    if (b == 0) return;   // wave-uniform
    const int lane = lane_id();
    const unsigned mine = (lane & 32) ? (unsigned)(b >> 32) : (unsigned)b;
    unsigned base = 0;
    if ((lane & 31) == 0 && mine != 0) base = atomicAdd(count, (unsigned)__popc(mine));
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)base, 0), hi = (unsigned)__builtin_amdgcn_readlane((int)base, 32);
    const unsigned pos = ((lane & 32) ? hi : lo) + (unsigned)__popc(mine & ((1u << (lane & 31)) - 1u));
    if (hit && pos < (unsigned)cap) hits[pos] = make_uint2(__float_as_uint(s), (unsigned)row);
}

// Key of a candidate (score, row): larger = ranks first under (score desc, row asc); 0 = none (a finite score's key is
// >= 0x00800000 and -inf's is 0x007fffff).  -0.0f would rank below +0.0f, but the scan's fmaf chains start from +0 and
// cannot produce it.
__device__ __forceinline__ uint64_t cand_key(float s, int32_t row) {
    return ((uint64_t)score_key(s) << 32) | (uint64_t)(0xffffffffu - (uint32_t)row);
}

// The emission of a group-max scan (kGroupMax), in the place of insert_candidates: a lane holds one (row, query) score.
// The row's group key comes from its tag; the lane's candidate key is folded into slot[g] of its query's table row
// (`table_q`, zeroed by the caller) by a 64-bit atomicMax, which a relaxed device-scope pre-read of the slot skips where
// the key cannot raise it.  A slot only grows, so a stale pre-read costs an extra atomic and never an answer: the table is
// the per-(query, group) maximum of the keys whatever order the workgroups ran in.  A matching row whose group key is
// >= n_groups is left out and sets *status.  Plain vector loads, stores and atomics.
__device__ __forceinline__ void emit_group_max(bool ok, float s, int row, int tag, int group_mask, int group_shift, int n_groups,
                                               unsigned long long* table_q, unsigned* status) {
    const unsigned g = (unsigned)(tag & group_mask) >> group_shift;
    // NaN and -inf never rank: such a row is no match, so it is in no group and sets no status (NaN's key would top every score's)
    if (!ok || !(s > -INFINITY)) return;
    if (g >= (unsigned)n_groups) {
        __hip_atomic_store(status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const unsigned long long key = cand_key(s, row);
    unsigned long long* slot = table_q + g;
    if (key > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(slot, key);
}

// The emission of a group-top scan (scan_grouptop.hip), in the place of insert_candidates: emit_group_max with a CHAIN of
// `levels` slots per (query, group) — level l of group g at table[slot_q + l * level_stride + g], all zeroed by the caller — that ends
// as the group's `levels` largest candidate keys, best first, whatever order the workgroups ran in.  The key enters level 0
// by a 64-bit atomicMax that returns what the slot held; the smaller of the two, the displaced one, moves down a level, until
// it falls into an empty slot or off the end.  Level 0 takes in every key and ends as their maximum; every other key is handed
// to level 1 exactly once (as the loser of one exchange), so level 1 ends as the second largest, and so on by induction.  Keys
// are unique (rows are distinct).  The pre-read of the LAST level skips a key that cannot be among the `levels` largest: slots
// only grow, so a stale value costs extra atomics and never an answer.  g: the row's group (>= 0); one >= n_groups on a
// matching row is left out and sets *status.  Plain vector loads and atomics, relaxed, agent scope.
__device__ __forceinline__ void emit_group_top(bool ok, float s, int row, int g, int n_groups, unsigned long long* table,
                                               unsigned slot_q, unsigned level_stride, int levels, unsigned* status) {
    // NaN and -inf never rank: such a row is no match, so it is in no group and sets no status
    if (!ok || !(s > -INFINITY)) return;
    if ((unsigned)g >= (unsigned)n_groups) {
        __hip_atomic_store(status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    unsigned long long key = cand_key(s, row);
    // the whole table is addressed by one 32-bit slot index (levels * nq * n_groups <= 2^25) from a wave-uniform base
    unsigned slot = slot_q + (unsigned)g;
    if (key <= __hip_atomic_load(table + (slot + (unsigned)(levels - 1) * level_stride), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    for (int l = 0; l < levels - 1; ++l, slot += level_stride) {
        const unsigned long long old = __hip_atomic_fetch_max(table + slot, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        key = old < key ? old : key;   // the displaced one moves down a level
        if (key == 0ull) return;       // it displaced an empty slot
    }
    // the last level: what it displaces falls off the end, so nothing is read back and the lane does not wait (with one level
    // this is emit_group_max's atomic)
    (void)__hip_atomic_fetch_max(table + slot, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The emission of a group-count scan (kGroupCount), in the place of insert_candidates: a half-wave holds one query's 32 rows
// of a tile, `hit` says which of them count (live, filters passed, a real query, score >= the query's threshold).  A hit
// whose group key is >= n_groups is left out and sets *status, as in emit_group_max.  Slot of a hit: q * n_groups + g of
// `count` (32-bit, zeroed by the caller) and of `best` (emit_group_max's table).  A document's chunks are adjacent rows, so the
// hits of a half usually share one group: where every hit lane of a half agrees with the half's first hit lane (ballot,
// readlane), that lane adds the half's number of hits once, as emit_range does; otherwise every hit lane adds 1.  Integer
// adds commute: the counters are a function of the input alone either way.  The best row is folded in exactly as
// emit_group_max does it.  Both tables are addressed by one 32-bit slot index (< 2^25) from wave-uniform bases.
// Plain vector loads, stores and atomics.
__device__ __forceinline__ void emit_group_count(bool hit, float s, int row, int tag, int q, int group_mask, int group_shift,
                                                 int n_groups, unsigned long long* best, unsigned* count, unsigned* status) {
    const unsigned g = (unsigned)(tag & group_mask) >> group_shift;
    const bool inside = g < (unsigned)n_groups;
    hit = hit && s > -INFINITY;   // NaN and -inf never rank: no hit, no status
    if (hit && !inside) __hip_atomic_store(status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    hit = hit && inside;
    const unsigned long long b = __ballot(hit);
    if (b == 0) return;   // wave-uniform
    const unsigned lo = (unsigned)b, hi = (unsigned)(b >> 32);
    // the first hit lane of each half (a half without hits: any lane of it, nothing is compared with its key)
    const int f_lo = __builtin_amdgcn_readfirstlane(lo ? __builtin_ctz(lo) : 0);
    const int f_hi = __builtin_amdgcn_readfirstlane(hi ? 32 + __builtin_ctz(hi) : 32);
    const unsigned g_lo = (unsigned)__builtin_amdgcn_readlane((int)g, f_lo), g_hi = (unsigned)__builtin_amdgcn_readlane((int)g, f_hi);
    const int lane = lane_id();
    const bool upper = (lane & 32) != 0;
    const unsigned long long d = __ballot(hit && g != (upper ? g_hi : g_lo));
    const bool shared = (upper ? (unsigned)(d >> 32) : (unsigned)d) == 0u;   // my half's hits are of one group
    if (!hit) return;
    const unsigned slot = (unsigned)q * (unsigned)n_groups + g;
    if (!shared)
        atomicAdd(count + slot, 1u);
    else if (lane == (upper ? f_hi : f_lo))
        atomicAdd(count + slot, (unsigned)__popc(upper ? hi : lo));
    const unsigned long long key = cand_key(s, row);
    if (key > __hip_atomic_load(best + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(best + slot, key);
}

// The emission of a top-hits scan (scan_tophits.hip), in the place of insert_candidates: emit_group_count's counters with
// emit_group_top's chain in the place of its one best-row slot — a terms aggregation whose buckets carry their `levels` best
// hits.  g is the row's group (>= 0; a key column, no tag field).  The count comes FIRST and is emit_group_count's half-wave
// logic to the letter: the chain's pre-read of the last level may skip the chain of a hit that cannot be among the bucket's
// `levels` best, never its count.  Count slot of a hit: q * n_groups + g; level l of the chain at table[q * n_groups + l *
// level_stride + g].  With one level the chain is emit_group_max's atomic: count and plane 0 end byte for byte as
// emit_group_count leaves them.  Everything is addressed by one 32-bit slot index (< 2^25) from wave-uniform bases.
// Plain vector loads, stores and atomics.
__device__ __forceinline__ void emit_group_count_top(bool hit, float s, int row, int g, int q, int n_groups, unsigned long long* table,
                                                     unsigned level_stride, int levels, unsigned* count, unsigned* status) {
    const bool inside = (unsigned)g < (unsigned)n_groups;
    hit = hit && s > -INFINITY;   // NaN and -inf never rank: no hit, no status
    if (hit && !inside) __hip_atomic_store(status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    hit = hit && inside;
    const unsigned long long b = __ballot(hit);
    if (b == 0) return;   // wave-uniform
    const unsigned lo = (unsigned)b, hi = (unsigned)(b >> 32);
    // the first hit lane of each half (a half without hits: any lane of it, nothing is compared with its key and it adds nothing)
    const int f_lo = __builtin_amdgcn_readfirstlane(lo ? __builtin_ctz(lo) : 0);
    const int f_hi = __builtin_amdgcn_readfirstlane(hi ? 32 + __builtin_ctz(hi) : 32);
    const unsigned g_lo = (unsigned)__builtin_amdgcn_readlane(g, f_lo), g_hi = (unsigned)__builtin_amdgcn_readlane(g, f_hi);
    const int lane = lane_id();
    const bool upper = (lane & 32) != 0;
    const unsigned long long d = __ballot(hit && (unsigned)g != (upper ? g_hi : g_lo));
    const bool shared = (upper ? (unsigned)(d >> 32) : (unsigned)d) == 0u;   // my half's hits are of one group
    if (!hit) return;
    const unsigned slot_q = (unsigned)q * (unsigned)n_groups;
    if (!shared)
        atomicAdd(count + (slot_q + (unsigned)g), 1u);
    else if (lane == (upper ? f_hi : f_lo))
        atomicAdd(count + (slot_q + (unsigned)g), (unsigned)__popc(upper ? hi : lo));
    // a hit lane from here on: in range and s > -inf, so emit_group_top neither drops it nor touches the status word
    emit_group_top(true, s, row, g, n_groups, table, slot_q, level_stride, levels, status);
}

// Half-wave sorted list: lanes 0..31 hold query A's best-first top-32, lanes 32..63 query B's.
struct TopList {
    float s;
    int i;
};

// The k-th best score of my half (lanes 0..31 / 32..63): two readlanes + a select, no LDS permute.
__device__ __forceinline__ float bcast_kth(float v, int k) {
    const int a = __builtin_amdgcn_readlane(__float_as_int(v), k - 1);
    const int b = __builtin_amdgcn_readlane(__float_as_int(v), 32 + k - 1);
    return __int_as_float((lane_id() & 32) ? b : a);
}

// Lane i <- lane i-1 across the whole wave (lane 0 keeps its value): one DPP move (wave_shr:1).
__device__ __forceinline__ int wave_shr1(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }

// Insert every lane's candidate (cs valid where cs > tau of its half) into the half-wave lists.
// Everything stays in registers / the scalar unit: the first version used __shfl_up / __shfl here, which
// hipcc lowers to ds_bpermute_b32 — three LDS round trips (~400 cycles) per inserted candidate.  A per-workgroup
// list takes ~k ln(n/k) (60 at k = 10, 3 900 rows) insertions per launch and the 8 waves meet at a barrier every
// two tiles, so the slowest wave's insertions were on every workgroup's critical path: with the ranking
// removed the B = 32 kernel ran 72 us (10 %) faster, with only the insertion removed 57 us
// (profiles/r02_scan_phase_experiments.txt).
__device__ __forceinline__ void insert_candidates(TopList& L, float& tau, float s, int row, int k) {
    unsigned long long mask = __ballot(s > tau);
    const int lane = lane_id();
    const int lpos = lane & 31;
    while (mask) {
        const int c = __builtin_ctzll(mask);
        mask &= mask - 1;
        const float cs = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), c));
        const int ci = __builtin_amdgcn_readlane(row, c);
        // straight-line body (bitwise predicates, selects): the short-circuit / nested-if form compiled to five
        // exec-mask branches per candidate
        const bool mine = ((lane ^ c) & 32) == 0;
        const bool better = (L.s > cs) | ((L.s == cs) & (L.i < ci));
        const int pos = __builtin_popcountll(__ballot(better & mine));
        const float us = __int_as_float(wave_shr1(__float_as_int(L.s)));
        const int ui = wave_shr1(L.i);
        const bool live = mine & (pos < k);          // a candidate that ranks behind the k kept changes nothing
        const bool take = live & (lpos == pos);
        const bool shift = live & (lpos > pos);
        L.s = take ? cs : (shift ? us : L.s);
        L.i = take ? ci : (shift ? ui : L.i);
        tau = bcast_kth(L.s, k);
        // candidates the raised threshold has just ruled out leave the queue (they would rank behind the k kept: same lists).
        // A workgroup's FIRST tile meets empty lists — all 64 lanes queue up — and on a small slab (an IVF's coarse scan, a
        // fine scan at nprobe 1, a 10 k-row index) that tile is the whole launch: 64 serial steps per part cost 5.5 us of a
        // 15 us launch however small k was (r03, scripts/microbench/scan_small.hip).
        mask &= __ballot(s > tau);
    }
}

// ---- bulk insertion: MANY candidates of one call at once (round 4) ------------------------------------------------------
// insert_candidates takes one candidate per step, ~200 cycles each, serially over the wave.  That is the right shape when a
// tile yields a handful of candidates per query (the flat scan behind a sample floor).  It is the wrong one where a tile is
// DENSE in candidates: an IVF's fine scan (a tile belongs to a list one or two of the batch's queries probe, nearly all of its
// 64 rows beat that workgroup's short list, and the one wave that ranks that query works through them while seven wait at
// the barrier: 6 us per 64-KiB tile of an int8 slab, scan_i8.hip), or any workgroup's first tile.  Here the half-wave's 32
// candidates are SORTED (worst first: a 15-stage bitonic network on DPP / v_permlane16_swap, both halves = both queries of
// the wave at once), compared lane by lane with the running list (best first: list ++ candidates is a bitonic sequence and the
// lane-wise winner its best 32) and re-sorted by the 5-stage bitonic merge: ~21 compare-exchange stages whatever the number of
// candidates — the same list the one-by-one insertion ends with ((score desc, row asc) is a total order).

// The lane exchange of that network and of the merge's (merge_topk.hip).
// One dword of lane (lane ^ STRIDE), in registers: DPP moves inside a row of 16 lanes (quad permutes for 1 and 2; 4 and 8 as a
// mirror of a mirror: half_mirror(i) = i ^ 7, quad_reverse(i) = i ^ 3, row_mirror(i) = i ^ 15), v_permlane16_swap /
// v_permlane32_swap across rows (swap(x, x) leaves the even rows / the lower half of x in every row of the first result and
// the odd rows / the upper half in the second: a lane's partner value is in the result its own row does not name).  Round 3:
// the 34 compare-exchange stages of a merge (merge_topk.hip) were 102 ds_bpermute round trips through the LDS crossbar.
template <int STRIDE>
__device__ __forceinline__ int xor_lane(int v, int lane) {
    static_assert(STRIDE == 1 || STRIDE == 2 || STRIDE == 4 || STRIDE == 8 || STRIDE == 16 || STRIDE == 32, "stride");
    if constexpr (STRIDE == 1) return __builtin_amdgcn_mov_dpp(v, 0xB1, 0xf, 0xf, true);          // quad_perm [1,0,3,2]
    if constexpr (STRIDE == 2) return __builtin_amdgcn_mov_dpp(v, 0x4E, 0xf, 0xf, true);          // quad_perm [2,3,0,1]
    if constexpr (STRIDE == 4)   // i ^ 4 = half_mirror(quad_reverse(i)): (i ^ 3) ^ 7
        return __builtin_amdgcn_mov_dpp(__builtin_amdgcn_mov_dpp(v, 0x1B, 0xf, 0xf, true), 0x141, 0xf, 0xf, true);
    if constexpr (STRIDE == 8)   // i ^ 8 = row_mirror(half_mirror(i)): (i ^ 7) ^ 15
        return __builtin_amdgcn_mov_dpp(__builtin_amdgcn_mov_dpp(v, 0x141, 0xf, 0xf, true), 0x140, 0xf, 0xf, true);
    if constexpr (STRIDE == 16) {
        const auto sw = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
        return (int)((lane & 16) ? sw[0] : sw[1]);
    }
    if constexpr (STRIDE == 32) {
        const auto sw = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
        return (int)((lane & 32) ? sw[0] : sw[1]);
    }
    return v;
}

template <int STRIDE>
__device__ __forceinline__ void top_cmpx(float& s, int& i, int lane, bool keep_better) {
    const float os = __int_as_float(xor_lane<STRIDE>(__float_as_int(s), lane));
    const int oi = xor_lane<STRIDE>(i, lane);
    const bool mine_better = (s > os) | ((s == os) & (i < oi));
    const bool take = mine_better != keep_better;
    s = take ? os : s;
    i = take ? oi : i;
}

template <int SIZE, int STRIDE>
__device__ __forceinline__ void top_sort_steps(float& s, int& i, int lane) {   // one level of the half-wave bitonic sort
    if constexpr (STRIDE > 0) {
        // blocks of SIZE alternate direction; the last level (SIZE == 32) runs WORST first in both halves
        const bool best_first = SIZE == 32 ? false : (lane & SIZE) == 0;
        const bool lower = (lane & STRIDE) == 0;
        top_cmpx<STRIDE>(s, i, lane, best_first == lower);
        top_sort_steps<SIZE, STRIDE / 2>(s, i, lane);
    }
}

// cs / ci: this lane's candidate, already (-inf, 0x7fffffff) where it may not rank.  Both halves (two queries) at once.
__device__ __forceinline__ void insert_candidates_bulk(TopList& L, float& tau, float cs, int ci, int k) {
    const int lane = lane_id();
    top_sort_steps<2, 1>(cs, ci, lane);
    top_sort_steps<4, 2>(cs, ci, lane);
    top_sort_steps<8, 4>(cs, ci, lane);
    top_sort_steps<16, 8>(cs, ci, lane);
    top_sort_steps<32, 16>(cs, ci, lane);
    // list (best first) ++ candidates (worst first) is bitonic: the lane-wise winners are its best 32, themselves bitonic
    const bool keep = (L.s > cs) | ((L.s == cs) & (L.i < ci));
    float s = keep ? L.s : cs;
    int i = keep ? L.i : ci;
    top_cmpx<16>(s, i, lane, (lane & 16) == 0);
    top_cmpx<8>(s, i, lane, (lane & 8) == 0);
    top_cmpx<4>(s, i, lane, (lane & 4) == 0);
    top_cmpx<2>(s, i, lane, (lane & 2) == 0);
    top_cmpx<1>(s, i, lane, (lane & 1) == 0);
    // entries behind the k kept are dropped, as the one-by-one insertion never stores them
    const bool kept = (lane & 31) < k;
    L.s = kept ? s : -INFINITY;
    L.i = kept ? i : 0x7fffffff;
    tau = bcast_kth(L.s, k);
}

// One call site for both shapes: the network when the call brings at least kBulkMin candidates, one by one below.
constexpr int kBulkMin = 8;
__device__ __forceinline__ void insert_candidates_auto(TopList& L, float& tau, float s, int row, int k) {
    const unsigned long long mask = __ballot(s > tau);
    if (__popcll(mask) >= kBulkMin) {
        const bool in = s > tau;
        insert_candidates_bulk(L, tau, in ? s : -INFINITY, in ? row : 0x7fffffff, k);
    } else if (mask) {
        insert_candidates(L, tau, s, row, k);
    }
}

}  // namespace rass
