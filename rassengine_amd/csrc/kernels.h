// kernels.h — internal launcher interface between the C-ABI layer (api_*.hip) and the
// gfx950 kernels.  Not part of the public ABI (include/rass_engine.h is).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rass {

constexpr int kMaxSampleGroups = 256;  // workgroups of a sample pass (ScanArgs::sample_best)

struct ScanArgs {
    const float* corpus;      // tile16-packed fp32 slab (see below), rows L2-normalised, zero padded past dim
    const int32_t* row_tag;   // [n_rows] or nullptr; -1 = tombstone, >= 0 = patientId code
    const float* q_padded;    // [16*NT][row_stride] normalised queries, zero rows past nq
    const int32_t* q_filter;  // [nq] or nullptr; -1 = no filter
    // Extended per-query filters (all nullptr for the plain scan; any non-null selects the EXT kernel variant):
    //   q_filter_mask[q]: a row matches when (tag & mask) == q_filter[q] (tag = patient code | doc_type << 24,
    //                     so one compare serves `term: patientId`, `term: doc_type` or both); nullptr = exact compare
    //   q_after_score/q_after_id[q]: continuation bound of a multi-pass top-k (k > 32): only rows that rank
    //                     strictly AFTER (score, global id) under (score desc, id asc) are eligible
    const int32_t* q_filter_mask = nullptr;
    const float* q_after_score = nullptr;
    const int64_t* q_after_id = nullptr;
    float* part_scores;       // [grid][nq][k]
    int64_t* part_ids;        // [grid][nq][k]
    int64_t row_stride;       // elements, multiple of 128
    int64_t id_base;          // added to local row ids
    int n_rows;
    int nq;
    int k;
    // IVF probe plan (all nullptr for the flat scan): work item i = slab tile work_tile[i] with
    // work_rows[i] valid rows, visible to the queries whose bit is set in work_mask[i]
    const int32_t* work_tile = nullptr;
    const int32_t* work_rows = nullptr;
    const uint32_t* work_mask = nullptr;
    const int32_t* n_work = nullptr;  // device scalar: number of work items
    // cross-index batch (all nullptr otherwise): item i scans tile work_tile[i] of the slab work_base[i] with the
    // row tags work_tags[i] (may be null per item); ids are rows of THAT slab
    const float* const* work_base = nullptr;
    const int32_t* const* work_tags = nullptr;
    // The sample floor (nullptr = none).  sample_best[32][kMaxSampleGroups] holds, for g < sample_groups, the best
    // score per query that workgroup g of a SAMPLE PASS found (the same scan over a small prefix of the slab, run
    // first with sample_pass = true, which writes exactly this array through part_scores).  Each wave of the big
    // scan takes, per query, the k-th largest of those as a floor: k different rows reach it, hence so does the
    // final k-th best, and rows scoring below it are dropped before the sorted insertion.  That insertion is where
    // the 32-query scan spends its non-MFMA time: every workgroup list otherwise takes ~k(1 + ln(rows/k))
    // insertions, ~70 at k = 10 over 3,900 rows, most of them in the first iterations.  Results do not depend on
    // the floor (rows tying with it are kept).
    const float* sample_best = nullptr;
    int sample_groups = 0;
    bool sample_pass = false;  // this launch IS the sample pass (flat, > 16 queries): same code, its own kernel name
    // XCD skew (0 = plain round-robin).  Workgroups land on XCD blockIdx % 8; measured on MI355X
    // (scripts/microbench/scan_tail.hip) the odd XCDs stream ~14 % slower than the even ones when
    // the scan is purely HBM-bound (B <= 16).  With skew s > 0 the even workgroups take s+1 items
    // for every s the odd ones take, so all of them finish together.  Needs an even grid.
    int xcd_skew = 0;
    // device scalar (nullptr = none): when it reads 0 every workgroup exits at once — the fp32 fallback of the certified
    // int8 mode (prefilter mode 3) is enqueued unconditionally and runs only when some query's certificate failed
    const int32_t* live_nq = nullptr;
    // Grouped flat scan (kFlatGroups; 0 = off): workgroups [g * wgs_per_group, (g + 1) * wgs_per_group) serve launch group
    // g — its 32 (zero-padded) queries at q_padded + g * q_group_stride, its lists at part_* + g * part_group_stride
    // ([wgs_per_group][nq][k], nq = 32 for every group), its filters at q_filter + 32 g.  No sample floor, no EXT.
    int wgs_per_group = 0;
    int64_t q_group_stride = 0, part_group_stride = 0;
    // Grouped IVF fine scan (kIvfGroups; work_tile != nullptr and wgs_per_group > 0): group g walks the work list at
    // work_* + g * work_group_stride with n_work[g] items; it has min(32, nq_total - 32 g) queries and writes dense lists
    // [wgs_per_group][that many][k] at part_* + g * part_group_stride.
    int64_t work_group_stride = 0;
    int nq_total = 0;
    // Range scan (kRange; range_count != nullptr selects it: flat scans only, no sample floor, no continuation bound, `k`
    // and part_* unused).  A row that is live and passes query q's filter is a HIT when its score >= range_thr[q] (a NaN
    // threshold matches nothing).  range_count[q * kRangeCountStride] (zeroed by the caller) ends as the exact number of
    // hits; the first range_cap of them to arrive are stored, unsorted, at range_hits[q * range_cap + ..] as (score bits,
    // row of this slab).  launch_range_finish turns that into the answer.
    union {
        const float* range_thr = nullptr;
        // The step kernel (scan_step.hip) only, never together with a range or group-count scan: floor[q] for every query of
        // the launch, ready-made (launch_step_floors: what the prologue of a scan selects from sample_best), or nullptr = none.
        // It shares range_thr's slot for the reason group_keys shares range_hits' (below).
        const float* step_floors;
    };
    unsigned* range_count = nullptr;
    union {
        uint2* range_hits = nullptr;
        const int32_t* group_keys;   // kGroupMaxKeys / kGroupCountKeys (below): never together with a range scan
    };
    int range_cap = 0;
    // Group-max scan (kGroupMax; group_table != nullptr selects it: flat scans only, no sample floor, no continuation bound,
    // `k` and part_* unused).  The group key of a row is (tag & group_mask) >> group_shift.  A row that is live and passes
    // query q's filter is folded into group_table[q * group_n + key] (zeroed by the caller; row_tag must not be null): the
    // slot ends as the largest candidate key (scan_core.h cand_key: score desc, row asc) of the group's matching rows, 0 =
    // none.  A matching row with key >= group_n is left out and sets *group_status (zeroed by the caller) to 1.
    // launch_group_select turns the table into the answer.
    unsigned long long* group_table = nullptr;
    unsigned* group_status = nullptr;
    int group_mask = 0, group_shift = 0, group_n = 0;
    int group_key_rows = 0;   // kGroupMaxKeys / kGroupCountKeys (below)
    // Allow-list scan (kAllow; allow != nullptr selects it: narrow rows, <= 32 zero-padded queries, a work list as for an IVF
    // probe — launch_allow_plan's —, plain or masked filters and the continuation bound; no sample floor).  Query q's word of
    // tile t is allow[q * allow_q_stride + t] (allow_q_stride = 0: one bitmap shared by every query); bit r of it allows row
    // 32 t + r.  A row ranks for q when it is live, passes q's filter and bound, and its bit is set.  Each wave reads the two
    // words of its two queries of a ranking step with scalar loads: they take no vector register and no LDS.
    const uint32_t* allow = nullptr;
    int64_t allow_q_stride = 0;
    // Group-count scan (kGroupCount; count_table != nullptr selects it, with group_table, group_status, group_mask / shift / n
    // and range_thr set as for the two scans above: flat scans only, no sample floor, no continuation bound, `k` and part_*
    // unused).  A row that is live, passes query q's filter and scores >= range_thr[q] (a NaN threshold matches nothing) is a
    // HIT: count_table[q * group_n + key] += 1 and its candidate key is folded into group_table[q * group_n + key] (both
    // zeroed by the caller).  A hit with key >= group_n is left out and sets *group_status to 1.  launch_group_count_select
    // turns the two tables into the answer.
    unsigned* count_table = nullptr;
    // Key-column grouping (kGroupMaxKeys / kGroupCountKeys; group_keys != nullptr selects them, with the fields of the group-max
    // or group-count scan set as above except group_mask / group_shift, which are not read).  The group of row r is
    // group_keys[r]: >= 0 the key, negative (RASS_KEY_NONE) = in no group.  A row without a group, or at or past
    // group_key_rows, is neither a match nor a hit and never touches *group_status; a key >= group_n on a matching row / a hit
    // sets it, as above.  row_tag may be null (no tombstones, no filters).  `allow` (optional, narrow rows only) restricts
    // query q to the rows whose bit is set in allow[q * allow_q_stride + tile], kAllow's test (the words are read through the
    // constant address space: these kernels write global memory, and a plain load would not come out scalar); the scan stays flat — every
    // tile is streamed whatever the bitmap holds (a plan-driven walk that skips tiles is not built).
    // The two fields live in the struct where it had room (group_keys shares range_hits' slot, group_key_rows fills the
    // padding behind group_n): the kernel argument block keeps its size and every older field its offset, so the kernels that
    // do not read them compile to the device code they had.
};
// The layout the comment above promises: the argument block of every scan kernel is these 312 bytes.
static_assert(sizeof(ScanArgs) == 312 && offsetof(ScanArgs, range_hits) == 240 && offsetof(ScanArgs, group_keys) == 240 &&
                  offsetof(ScanArgs, range_cap) == 248 && offsetof(ScanArgs, group_n) == 280 &&
                  offsetof(ScanArgs, group_key_rows) == 284 && offsetof(ScanArgs, allow) == 288 &&
                  offsetof(ScanArgs, count_table) == 304,
              "ScanArgs grew or moved a field: every scan kernel's device code changes with it");
constexpr int kRangeCountStride = 32;   // one 128-byte line per query's counter: every workgroup adds to all of them
constexpr int kRangeMaxHits = 4096;     // = RASS_MAX_K_MULTIPASS: 4 096 64-bit sort keys are range_finish's 32 KiB of LDS

bool scan_supported_stride(int64_t row_stride);
hipError_t launch_scan_topk_f32(const ScanArgs& a, int grid, hipStream_t stream);
// Two consecutive FULL launch groups of a flat fp32 scan in one corpus pass (scan_topk_f32_pair_kernel): a.nq = 64; queries
// 0..31 are addressed as launch_scan_topk_f32 would address group g's (q_padded, q_filter, sample_best, part_*: lists
// [grid][32][k]), queries 32..63 at q_padded + q_group_stride, q_filter + 32, sample_best + 32 * kMaxSampleGroups and
// part_* + part_group_stride.  Same scores and lists, bit for bit, as the two launches it replaces.  No EXT, no work list.
bool scan_pair_supported_stride(int64_t row_stride);
hipError_t launch_scan_topk_f32_pair(const ScanArgs& a, int grid, hipStream_t stream);
// A run of 1..kStepMaxPairs consecutive pairs in ONE launch (scan_step.hip, scan_topk_f32_step_kernel): `a` as for the pair
// launch of the run's first pair, except that a.nq_total = 64 * pairs, a.sample_best is not read and the floors come ready-made,
// one per query of the run, from a.step_floors (launch_step_floors; nullptr: none).  Pair j reads and writes where the pair
// launch with q_padded + 2 j * q_group_stride, q_filter + 64 j, part_* + 2 j * part_group_stride would: the same lists, bit for
// bit.  grid <= the slab's tiles (scan_grid gives that for a slab with a row).
constexpr int kStepMaxPairs = 16;
hipError_t launch_scan_topk_f32_step(const ScanArgs& a, int grid, hipStream_t stream);

// ---- boosted scan (scan_boost.hip; the flat pair loop it shares with the function-score scan: scan_flat.h):
// exact top-k of fused = boost[q] * T(cos) + bonus[q][row] for one launch group.
// `scan` carries what a flat EXT launch of launch_scan_topk_f32 would (corpus, row_tag, q_padded [32][row_stride] zero-padded,
// q_filter / q_filter_mask, q_after_score / q_after_id — the continuation bound, on the FUSED score and the slab row —,
// part_* [grid][nq][k], row_stride 128 * {1..8}, n_rows >= 1, nq <= 32, k <= 32, id_base 0: the lists hold slab rows); every
// other field of it stays at its default.  bonus: query q's column at bonus + q * bonus_q_stride (0: one column shared by
// every query), bonus_rows values each (<= bonus_q_stride where that is set); a row at or past bonus_rows reads 0.
// bonus_bytes = 4 * ((nq - 1) * bonus_q_stride + bonus_rows) <= kBoostMaxBonusBytes: the records of the kernel's one buffer
// descriptor.  boost [nq] or nullptr (1.0).  transform 0: T(s) = s; 1: T(s) = 1 / (2 - s).  A row ranks when it is live,
// passes the filter and the bound, s > -inf and fused > -inf; order (fused desc, row asc).  No sample floor.
// ScanArgs itself is untouched: the other scan kernels' argument block keeps its size and offsets.
constexpr int64_t kBoostMaxBonusBytes = 0x7fffffff;
struct BoostArgs {
    ScanArgs scan;
    const float* bonus = nullptr;
    int64_t bonus_q_stride = 0;
    int64_t bonus_rows = 0;
    unsigned bonus_bytes = 0;
    int transform = 0;
    const float* boost = nullptr;
};
hipError_t launch_scan_boost_f32(const BoostArgs& a, int grid, hipStream_t stream);

// ---- group-top scan (scan_grouptop.hip): the group_size best rows of every (query, group) for one launch group, in one pass.
// `scan` carries what a key-column group-max launch of launch_scan_topk_f32 would (corpus, row_tag or nullptr, q_padded
// [32][row_stride] zero-padded, q_filter / q_filter_mask, group_keys / group_key_rows, group_n, group_status, allow /
// allow_q_stride, row_stride 128 * {1..8}, n_rows >= 1, nq <= 32); every other field of it stays at its default.
// scan.group_table is LEVEL-MAJOR, [group_size][nq][group_n] 64-bit slots zeroed by the caller: level l of (q, g) at
// group_table[l * level_stride + q * group_n + g], level_stride >= nq * group_n.  It ends holding, per (q, g), the candidate
// keys (scan_core.h cand_key) of the group's matching rows from the largest down, 0 past the group's last row: plane 0 is what
// the group-max scan leaves, so launch_group_select reads it as it stands.  1 <= group_size <= kGroupHitsMaxSize and
// group_n * group_size <= kGroupMaxGroups (below).  No ranking: no TopList, no sample floor, no continuation bound.
// ScanArgs itself is untouched.
constexpr int kGroupHitsMaxSize = 16;
struct GroupTopArgs {
    ScanArgs scan;
    int64_t level_stride = 0;
    int group_size = 0;
};
hipError_t launch_scan_grouptop_f32(const GroupTopArgs& a, int grid, hipStream_t stream);

// ---- stats scan (scan_stats.hip, on scan_flat.h's loop): per (query, group), the hits of a key-column group-count scan AND
// the count / sum / min / max of an int32 value column over them, for one launch group, in one pass.
// `scan` carries what a key-column group-count launch of launch_scan_topk_f32 would (corpus, row_tag or nullptr, q_padded
// [32][row_stride] zero-padded, q_filter / q_filter_mask, range_thr [nq], group_keys / group_key_rows, group_n, group_status,
// allow / allow_q_stride, row_stride 128 * {1..8}, n_rows >= 1, nq <= 32) except count_table, which stays nullptr as every
// other field of it does: the counters are `count` below.  group_keys == nullptr: every row < group_key_rows has key 0 (the
// global form; group_n is then 1).  values: the value of row r is values[r], kStatsMissing = no value; nullptr: every row
// reads kStatsMissing (a column that was never set) and no memory request is made.
// The table is PLANE-MAJOR, six arrays of [nq][group_n] zeroed by the caller, slot q * group_n + g:
//   scan.group_table  u64  the best hit's candidate key (scan_core.h cand_key), as the group-count scan folds it
//   count             u32  hits
//   vcount            u32  hits with a value
//   sum               i64  the sum of those values (|v| < 2^31 and < 2^31 rows: it cannot overflow)
//   vmax              u32  stats_bias(largest value), stats_bias(v) = (uint32)v ^ 0x80000000: order-preserving, under atomicMax
//   vmin              u32  ~stats_bias(smallest value), under atomicMax too
// vcount == 0 says that vmin / vmax hold no value: the all-zero table is the empty table.  group_table and count end byte for
// byte as a kGroupCountKeys scan leaves them, so launch_group_count_select reads them as they stand.  A hit with key >=
// group_n is left out and sets *group_status.  ScanArgs itself is untouched.
constexpr int32_t kStatsMissing = INT32_MIN;   // = RASS_ATTR_MISSING
__host__ __device__ inline unsigned stats_bias(int32_t v) { return (unsigned)v ^ 0x80000000u; }
__host__ __device__ inline int32_t stats_unbias(unsigned u) { return (int32_t)(u ^ 0x80000000u); }
struct StatsArgs {
    ScanArgs scan;
    const int32_t* values = nullptr;
    unsigned* count = nullptr;
    unsigned* vcount = nullptr;
    long long* sum = nullptr;
    unsigned* vmin = nullptr;
    unsigned* vmax = nullptr;
};
hipError_t launch_scan_stats_f32(const StatsArgs& a, int grid, hipStream_t stream);

// ---- top-hits scan (scan_tophits.hip, on scan_flat.h's loop): per (query, group), the hits of a key-column group-count scan
// AND the `top_hits` best of them, for one launch group, in one pass: a terms aggregation with a top_hits sub-aggregation.
// `scan` carries what a key-column group-count launch of launch_scan_topk_f32 would (see StatsArgs above; group_keys is not
// nullptr here) except count_table, which stays nullptr: the counters are `count` below.
//   scan.group_table  u64  LEVEL-MAJOR [top_hits][nq][group_n] as GroupTopArgs' table: level l of (q, g) at
//                          group_table[l * level_stride + q * group_n + g], level_stride >= nq * group_n.  Per (q, g) the
//                          candidate keys (scan_core.h cand_key) of the group's HITS from the largest down, 0 past the last
//   count             u32  [nq][group_n] hits
// all zeroed by the caller.  Plane 0 and count end byte for byte as a kGroupCountKeys scan leaves its two tables, so
// launch_group_count_select and launch_group_select (over plane 0: only hits are in it) read them as they stand, and
// launch_group_hits_finish runs behind either.  1 <= top_hits <= kGroupHitsMaxSize, group_n * top_hits <= kGroupMaxGroups.
// A hit with key >= group_n is left out and sets *group_status.  ScanArgs itself is untouched.
struct TopHitsArgs {
    ScanArgs scan;
    unsigned* count = nullptr;
    int64_t level_stride = 0;
    int top_hits = 0;
};
hipError_t launch_scan_tophits_f32(const TopHitsArgs& a, int grid, hipStream_t stream);

// ---- bonus columns (bonus.hip): the dense fp32 columns the boosted scan adds.  A column block is [n_bonus][stride] floats.
// Plain vector loads and stores, no atomics.
// bonus[q_of[i] * stride + rows[i]] = that value + values[i] (one rounded add) for i < n.  The (q, row) pairs must be UNIQUE
// within a call and in range (the host entry checks; a device caller's duty): each cell has one writer.
hipError_t launch_bonus_scatter(const int32_t* q_of, const int64_t* rows, const float* values, int64_t n, float* bonus, int64_t stride,
                                hipStream_t stream);
// Weighted clauses over the attribute columns for one launch group of nq <= 32 bonus columns.  A clause {col, lo, hi, negate}
// holds for a row as attr.hip's does: v = col[c][row] is not INT32_MIN and lo <= v <= hi, inverted under negate; a NULL column
// reads as INT32_MIN everywhere.  clauses[q_off[q] .. q_off[q + 1]) are query q's, in the CALLER'S list order (the host sorts
// by query, stably); weights[j] belongs to clauses[j].  Per (query, row < n_rows): b = 0 (add = 0) or the cell's value (add =
// 1), then b = b + weight (one rounded add each) for every clause of the query that holds, in that order.  Tombstoned rows
// are written like any other.  Cells [n_rows, stride) are left alone.
struct BonusClauseArgs {
    const int32_t* col[8] = {};      // kAttrCols
    const int4* clauses = nullptr;
    const float* weights = nullptr;
    const int32_t* q_off = nullptr;  // DEVICE int32 [nq + 1], q_off[0] = 0
    int64_t n_rows = 0;
    float* bonus = nullptr;
    int64_t stride = 0;
    int nq = 0, add = 0;
};
hipError_t launch_bonus_clauses(const BonusClauseArgs& a, hipStream_t stream);
// bonus[q][r] = -inf where bit r of bitmap q (allow + q * allow_q_stride; 0: one shared bitmap) is clear, r < n_rows, q < n_bonus.
hipError_t launch_bonus_mask(float* bonus, int n_bonus, int64_t stride, int64_t n_rows, const uint32_t* allow, int64_t allow_q_stride,
                             hipStream_t stream);

// ---- function-score scan (scan_fscore.hip, on scan_flat.h's loop): exact top-k of fused = combine(boost[q] * T(cos),
// fn[q][row]) for one launch group.  `scan`, `boost` and `transform` as in BoostArgs.  fn: query q's function column at fn + q * fn_q_stride (0: one
// column shared by every query), fn_rows values each — fn_rows must equal scan.n_rows (no "rows past the column" here);
// fn_bytes = 4 * ((nq - 1) * fn_q_stride + fn_rows) <= kBoostMaxBonusBytes.  mode: RASS_COMBINE_* (0 sum a + f, 1 multiply
// a * f, 2 avg (a + f) * 0.5f, 3 max f > a ? f : a, 4 min f < a ? f : a, 5 replace f), every operation rounded on its own.
// min_score [nq] or nullptr: a row ranks for q only with T(cos) >= min_score[q] (-inf: no gate).  A row ranks when the boosted
// scan's conditions hold (on this fused score), the gate passes and f > -inf (a NaN or -inf cell excludes the row in EVERY
// mode); order (fused desc, row asc).  No sample floor.
constexpr int kCombineModes = 6;
struct FscoreArgs {
    ScanArgs scan;
    const float* fn = nullptr;
    int64_t fn_q_stride = 0;
    int64_t fn_rows = 0;
    unsigned fn_bytes = 0;
    int transform = 0;
    int mode = 0;
    const float* boost = nullptr;
    const float* min_score = nullptr;
};
hipError_t launch_scan_fscore_f32(const FscoreArgs& a, int grid, hipStream_t stream);

// ---- function columns (score_fn.hip): a column block [nq][stride] filled from function records over the attribute columns,
// for one launch group of nq <= 32 columns.  recs[q_off[q] .. q_off[q + 1]) are column q's functions in the caller's list
// order.  kind 0 gauss exp(d * d * c), 1 exp exp(d * c), 2 linear max(0, (c - d) / c) with d = max(0, |v - p0| - p1) and c the
// host-derived constant (1.0 on a missing value); 3 field_value_factor modifier(p0 * v) (v = `missing` on a missing value;
// NaN there: the function does not apply); 4 weight 1.0.  filter: -1 or a bitmap index into filters[.][words]; a function
// applies where its bit is set.  A function's value is weight * kind(v); the applying ones are folded in list order by
// score_mode (0 multiply, 1 sum, 2 avg = sum(value) / sum(weight), 3 first, 4 max, 5 min; max / min as compare and select),
// the result capped as value > max_boost ? max_boost : value; no applying function: 1.0.  ALL of it in double, rounded to
// fp32 once at the store.  Rows [0, n_rows) of each column are written, tombstoned rows too; the padding is left alone.
struct ScoreFnRec {
    int32_t kind, col, filter, modifier;
    double weight, p0, p1, c, missing;
};
struct ScoreFnArgs {
    const int32_t* col[8] = {};      // kAttrCols
    const ScoreFnRec* recs = nullptr;
    const int32_t* q_off = nullptr;  // DEVICE int32 [nq + 1]
    const uint32_t* filters = nullptr;
    int64_t words = 0;
    int64_t n_rows = 0;
    float* out = nullptr;
    int64_t stride = 0;
    int nq = 0, score_mode = 0;
    double max_boost = 0;
};
hipError_t launch_score_fn(const ScoreFnArgs& a, hipStream_t stream);

// [n_lists][nq][k] sorted candidate lists -> [nq][k]; n_lists * k <= kMergeMaxCandidates.
constexpr int kMergeMaxCandidates = 8192;
// `groups` (optional): ONE launch merges the lists of several launch groups of <= size queries each; nq is then
// the total query count, blockIdx / size the group, and every pointer advances by its *_stride per group (in
// elements).  lists_are_dense: a group's lists are [n_lists][nq_g][k] with nq_g its own query count (the scan's
// per-workgroup lists); otherwise the caller's list strides hold for every group (gathered packed records).
struct MergeGroups {
    int size = 0;  // 0 = ungrouped
    int nq_total = 0;
    bool lists_are_dense = false;
    int64_t score_stride = 0, id_stride = 0, out_score_stride = 0, out_id_stride = 0;
};
hipError_t launch_merge_topk(const float* scores, const int64_t* ids, int n_lists, int nq, int k,
                             float* out_scores, int64_t* out_ids, hipStream_t stream,
                             const int64_t* id_map = nullptr, int64_t score_list_stride = 0,
                             int64_t id_list_stride = 0, const MergeGroups* groups = nullptr,
                             const int32_t* live_nq = nullptr);   // as ScanArgs::live_nq: 0 = every workgroup exits

// The answer of a range scan, one workgroup per query (merge_topk.hip).  total[q] = count[q].  count <= cap: the emitted pairs
// sorted (score desc, row asc) into out_scores / out_ids [nq][cap], ids = id_map[row] (ascending with the row) or id_base +
// row, the slots past the end (-inf, -1).  count > cap: which pairs were stored depended on timing — the whole list is
// (-inf, -1) and the total says why.
hipError_t launch_range_finish(const unsigned* count, const uint2* hits, int nq, int cap, int64_t id_base, const int64_t* id_map,
                               float* out_scores, int64_t* out_ids, int64_t* total, hipStream_t stream);

// The answer of a group-max scan, one workgroup per query (group_topk.hip).  table [nq][n_groups] holds each group's best
// candidate key (0 = no matching row).  total[q] = the number of non-zero slots.  The k largest keys (all of them where
// total <= k), best first: out_scores / out_ids / out_groups [nq][k] = the key's score, id_map[row] (ascending with the row)
// or id_base + row, and the slot index; (-inf, -1, -1) past the end.  1 <= k <= kGroupMaxK.  *out_status = the scan's status
// word (ScanArgs::group_status) as 0 / 1.
constexpr int kGroupMaxK = 4096;          // = RASS_MAX_K_MULTIPASS: the selected keys and their slots are 48 KiB of LDS
constexpr int kGroupMaxGroups = 1 << 20;  // the exclusive bound of a group key: a 32-query table is 256 MiB
hipError_t launch_group_select(const unsigned long long* table, int nq, int n_groups, int k, int64_t id_base, const int64_t* id_map,
                               float* out_scores, int64_t* out_ids, int32_t* out_groups, int64_t* total, const unsigned* status,
                               int32_t* out_status, hipStream_t stream);
// The answer of a group-count scan, by the same kernel.  counts / best [nq][n_groups]: each group's number of hits and its best
// candidate key.  n_buckets[q] = the number of non-zero counters, total_hits[q] = their sum.  The `size` first buckets (all of
// them where n_buckets <= size) under (count desc, group asc): out_groups / out_counts / out_scores / out_ids [nq][size] = the
// slot index, its counter, and the score and id of its best row as above; (-1, 0, -inf, -1) past the end.
// 1 <= size <= kGroupMaxK.  With both tables a 32-query group at kGroupMaxGroups is 384 MiB.
hipError_t launch_group_count_select(const unsigned* counts, const unsigned long long* best, int nq, int n_groups, int size, int64_t id_base,
                                     const int64_t* id_map, int32_t* out_groups, int64_t* out_counts, float* out_scores, int64_t* out_ids,
                                     int64_t* n_buckets, int64_t* total_hits, const unsigned* status, int32_t* out_status,
                                     hipStream_t stream);
// The inner hits of a group-top scan (scan_grouptop.hip) behind launch_group_select over plane 0 of its table, one workgroup
// per query.  table is level-major [group_size][nq][n_groups]; groups [nq][k] is what the select wrote (-1 past the end).
// out_scores / out_ids [nq][k][group_size] = levels 0 .. group_size - 1 of each selected slot, decoded and translated as the
// select does; (-inf, -1) past a group's last row and for a missing group.  They may overlap what the select wrote as
// out_scores / out_ids: neither is read.  cap_scores / cap_ids [nq][k] (both or neither; k * group_size <= kGroupMaxK): the k
// largest of those k * group_size keys, best first under (score desc, row asc), (-inf, -1) past the end.
// *out_status = the scan's status word as 0 / 1; with `accumulate` it is only ever raised (a call's later launch groups).
hipError_t launch_group_hits_finish(const unsigned long long* table, int nq, int n_groups, int k, int group_size, int64_t id_base,
                                    const int64_t* id_map, const int32_t* groups, float* out_scores, int64_t* out_ids,
                                    float* cap_scores, int64_t* cap_ids, const unsigned* status, int32_t* out_status, bool accumulate,
                                    hipStream_t stream);
// The answer of a stats scan (StatsArgs above), in two launches (group_topk.hip).
// launch_group_stats_select: launch_group_count_select's outputs with the buckets ordered by `order_by` (kStatsBy*), descending
// or ascending.  kStatsByCount descending IS launch_group_count_select, the same kernel.  Otherwise the select's key of slot g
// with count > 0 is  1 << 53 | has_value << 52 | metric << 20 | (2^20 - 1 - g),  metric = the counter, vcount, or the biased
// min / max of the slot, complemented for ascending order: the buckets without a value (vcount == 0; never under kStatsByCount)
// come after every bucket that has one in both directions, and ties break by group ascending.  n_buckets / total_hits as there.
// launch_group_stats_gather: for the buckets the select listed (groups [nq][size], -1 past the end) the decoded planes,
// out_vcounts / out_sums (int64) and out_mins / out_maxs (int32) [nq][size]; (0, 0, 0, 0) past the end and for a bucket
// without a value.
enum StatsOrder { kStatsByCount = 0, kStatsByValueCount = 1, kStatsByMin = 2, kStatsByMax = 3 };
hipError_t launch_group_stats_select(const unsigned* counts, const unsigned long long* best, const unsigned* vcount, const unsigned* vmin,
                                     const unsigned* vmax, int order_by, bool descending, int nq, int n_groups, int size, int64_t id_base,
                                     const int64_t* id_map, int32_t* out_groups, int64_t* out_counts, float* out_scores, int64_t* out_ids,
                                     int64_t* n_buckets, int64_t* total_hits, const unsigned* status, int32_t* out_status,
                                     hipStream_t stream);
hipError_t launch_group_stats_gather(const int32_t* groups, const unsigned* vcount, const long long* sum, const unsigned* vmin,
                                     const unsigned* vmax, int nq, int n_groups, int size, int64_t* out_vcounts, int64_t* out_sums,
                                     int32_t* out_mins, int32_t* out_maxs, hipStream_t stream);
// The counters of a top-hits scan (TopHitsArgs above) behind launch_group_select over plane 0 of its table (the buckets
// ordered by their best hit), one workgroup per query.  groups [nq][size] is what the select wrote (-1 past the end);
// out_counts [nq][size] = the listed buckets' counters, 0 past the end; total_hits[q] = the sum of the query's counters.
hipError_t launch_group_counts_gather(const int32_t* groups, const unsigned* counts, int nq, int n_groups, int size,
                                      int64_t* out_counts, int64_t* total_hits, hipStream_t stream);

// ---- allow-list search (allow.hip): row bitmaps, their work list, and the store of a pass.  A bitmap is uint32 words, bit
// (r & 31) of word r >> 5 allows row r.  Plain vector loads, stores and atomics.
// allow[row >> 5] |= 1 << (row & 31) for the n ids of `rows` that lie in [0, n_rows); duplicates are fine.  The caller zeroes `allow`.
hipError_t launch_allow_from_rows(const int64_t* rows, int64_t n, int64_t n_rows, uint32_t* allow, hipStream_t stream);
// The words of rows [0, n_rows): bit set where the row is live (tag != -1) and (tag & mask) is one of the n_values ASCENDING
// `values` (binary search; the set sits in LDS up to kAllowLdsValues of them).  Every word below ceil(n_rows / 32) is written.
constexpr int kAllowLdsValues = 2048;
hipError_t launch_allow_from_tag_values(const int32_t* tags, int64_t n_rows, const int32_t* values, int n_values, int32_t mask,
                                        uint32_t* allow, hipStream_t stream);
// The work list of one launch group of nq <= 32 queries over the tiles of n_rows rows, tiles ASCENDING (a workgroup must meet
// rows in ascending order: the insertion's tie rule): one item per tile in which some query has a bit set below n_rows, its
// mask the queries that do.  Word of (q, t): allow[q * q_stride + t], q_stride = 0 for a shared bitmap.  *n_work = the count.
// workspace: allow_plan_workspace_bytes(n_rows).  Two launches; no workgroup waits on another.
size_t allow_plan_workspace_bytes(int64_t n_rows);
hipError_t launch_allow_plan(const uint32_t* allow, int64_t q_stride, int nq, int64_t n_rows, int32_t* work_tile, int32_t* work_rows,
                             uint32_t* work_mask, int32_t* n_work, void* workspace, hipStream_t stream);
// One pass of a k > 32 search: the pass's merged lists [nq][kk] (scores, slab rows; -1 = none) go to out[q][kdone .. kdone + kk)
// of the [nq][k] answer, ids = id_map[row] or id_base + row, (-inf, -1) where there is none; after_*[q] = the pass's last hit
// as the next pass's continuation bound (score, row), or (-inf, INT64_MAX) when the pass came back short.
hipError_t launch_allow_store(const float* scores, const int64_t* rows, int nq, int kk, int k, int kdone, int64_t id_base,
                              const int64_t* id_map, float* out_scores, int64_t* out_ids, float* after_s, int64_t* after_i,
                              hipStream_t stream);
// counts[b] = the set bits of bitmap b (allow + b * q_stride) below n_rows, b < n_bitmaps <= 65 535; counts is device int64.
hipError_t launch_allow_count(const uint32_t* allow, int64_t q_stride, int n_bitmaps, int64_t n_rows, int64_t* counts, hipStream_t stream);

// ---- an IVF probe within a row bitmap (ivf_allow.hip): the probe plan of ONE launch group (plan_probe_kernel's work list of
// <= max_items items over 32-row tiles, *n_work of them) meets a bitmap over SOURCE rows (query q's words at allow + q *
// q_stride, q_stride = 0: one shared bitmap; `words` uint32 each).  For every item and every q < nq the slab-order word goes
// to slab_allow[q * slab_q_stride + tile] (a shared bitmap: one word per tile and slab_q_stride = 0; else slab_q_stride >=
// every tile index + 1): bit r = the caller's bit of source row slab_ids[32 * tile + r], 0 where r >= the item's rows, the
// position is padding (-1), the row lies at or past 32 * words, or the item's mask does not name q — what ScanArgs::allow
// takes with the slab as the corpus.  work_mask[i] is narrowed in place to the queries whose word is non-zero; the items
// that keep a query go, in their (ascending tile) order, to out_tile / out_rows / out_mask, *out_n = their number,
// *scanned_rows = the sum of their rows.  workspace: ivf_allow_workspace_bytes(max_items).  Two launches; no workgroup waits
// on another.  Plain vector loads, stores, ballots and atomics.
size_t ivf_allow_workspace_bytes(int64_t max_items);
hipError_t launch_ivf_allow_words(const int32_t* work_tile, const int32_t* work_rows, uint32_t* work_mask, const int32_t* n_work,
                                  int64_t max_items, const int64_t* slab_ids, const uint32_t* allow, int64_t q_stride, int64_t words,
                                  int nq, uint32_t* slab_allow, int64_t slab_q_stride, int32_t* out_tile, int32_t* out_rows,
                                  uint32_t* out_mask, int32_t* out_n, int64_t* scanned_rows, void* workspace, hipStream_t stream);
// *accum += *add_from (nullptr: nothing) + work_rows[0] + ... + work_rows[min(*n_work, max_items) - 1] (both nullptr: nothing).
hipError_t launch_work_rows_add(const int32_t* work_rows, const int32_t* n_work, int64_t max_items, const int64_t* add_from, int64_t* accum,
                                hipStream_t stream);

// ---- attribute predicates (attr.hip): clauses over int32 columns -> the bitmaps of one launch group of nq <= 32 queries.
// A clause {query, lo, hi, negate} of column c holds for row r when v = col[c][r] is not INT32_MIN and lo <= v <= hi, inverted
// under negate; a NULL column reads as INT32_MIN everywhere.  clauses[col_off[c] .. col_off[c + 1]) are column c's
// (col_off[0] = 0).  Bit q of a live row (tags[r] != -1, r < n_rows) = all (mode_any = 0) or any (1) of q's clauses hold; a
// query without a clause gets every live row under all, none under any.  Words [0, ceil(span_rows / 32)) of bitmap q at allow +
// q * q_stride are written: combine 0 = replace, 1 = and, 2 = or with what they hold; positions in [n_rows, span_rows)
// contribute 0 bits, so span_rows = 32 * words clears a replace / and target whole and span_rows = n_rows leaves an or
// target's surplus alone.  span_rows >= n_rows.
constexpr int kAttrCols = 8;   // = RASS_MAX_ATTRS
struct AttrArgs {
    const int32_t* tags = nullptr;
    const int32_t* col[kAttrCols] = {};
    const int4* clauses = nullptr;
    int col_off[kAttrCols + 1] = {};
    int64_t n_rows = 0, span_rows = 0;
    uint32_t* allow = nullptr;
    int64_t q_stride = 0;
    int nq = 0, mode_any = 0, combine = 0;
};
hipError_t launch_attr_clauses(const AttrArgs& a, hipStream_t stream);
// dst[i] = dst[i] & src[i] (op 1), | src[i] (2) or & ~src[i] (3) for i < words: two bitmaps of equal length, dst != src.
hipError_t launch_allow_combine(uint32_t* dst, const uint32_t* src, int64_t words, int op, hipStream_t stream);

// ---- key columns (group_keys.hip): the group of every row as int32 keys[n_keys], >= 0 the group, -1 (RASS_KEY_NONE) none; what
// ScanArgs::group_keys takes.  col: an attribute column of n_rows <= n_keys values (nullptr: all missing); keys[n_rows .. n_keys)
// = -1; missing_key >= -1 is the key of a missing value (INT32_MIN).  The tags are not read.  Plain vector loads and stores.
// key = col[r] - base where that lies in [0, INT32_MAX] (computed in 64 bits), else -1.
hipError_t launch_keys_from_attr(const int32_t* col, int64_t n_rows, int64_t n_keys, int32_t base, int32_t missing_key, int32_t* keys,
                                 hipStream_t stream);
// key = j where edges[j] <= col[r] < edges[j + 1], -1 outside [edges[0], edges[n_edges - 1]): `edges` is a DEVICE array of
// 2 <= n_edges <= kKeyMaxEdges strictly ascending values (the caller checks the order), held in LDS and binary searched.
constexpr int kKeyMaxEdges = 4097;   // = RASS_MAX_KEY_EDGES: RASS_MAX_K_MULTIPASS buckets
hipError_t launch_keys_from_attr_edges(const int32_t* col, int64_t n_rows, int64_t n_keys, const int32_t* edges, int n_edges,
                                       int32_t missing_key, int32_t* keys, hipStream_t stream);
// key = (tags[r] & mask) >> ctz(mask) for a live row, -1 for a tombstone: the group of the tag-keyed searches.  mask > 0.
hipError_t launch_keys_from_tag(const int32_t* tags, int64_t n_rows, int64_t n_keys, int32_t mask, int32_t* keys, hipStream_t stream);
// out[0] / out[1] = min / max and out[2..3] (one 64-bit count) over the values of col that are not missing in rows whose tag is
// not -1; the caller has set out to {INT32_MAX, INT32_MIN, 0, 0}.  col == nullptr: out is left as it is.
hipError_t launch_attr_minmax(const int32_t* col, const int32_t* tags, int64_t n_rows, int32_t* out, hipStream_t stream);

// ---- diversified (MMR) search (mmr.hip): the Gram matrices of short row lists and the greedy selection
constexpr int kMmrMaxFetch = 128;   // = RASS_MAX_MMR_FETCH: rows per list, candidates per query (two per lane of one wave)
// out[l][i][j] = the fp32 dot product of slab rows rows[l][i] and rows[l][j] (whole rows: `stride` columns, the padding is
// zero), l < n_lists, i, j < list_len <= kMmrMaxFetch.  An ordinal < 0 or >= n_rows, or a row whose tag is -1 (tags may be
// nullptr: no tombstones), is padding: +0.0 in its whole row and column.  One k-ordered v_mfma_f32_16x16x4_f32 chain per
// element, the same whatever n_lists and list_len are; out is bitwise symmetric.  The rows are read straight from the tile16
// slab: no workspace.
hipError_t launch_rows_gram(const float* slab, int64_t stride, const int32_t* tags, int64_t n_rows, const int64_t* rows,
                            int64_t n_lists, int list_len, float* out, hipStream_t stream);
// The greedy MMR selection of include/rass_engine.h (rass_index_search_mmr), one wave per query: cand_s / cand_rows
// [nq][fetch_k] (score desc; rows -1 past the candidates), gram [nq][fetch_k][fetch_k], lambda [nq] -> out_scores / out_ids /
// out_rank (may be nullptr) [nq][k] in selection order, ids = id_map[row] or id_base + row, (-inf, -1, -1) past the end.
hipError_t launch_mmr_select(const float* cand_s, const int64_t* cand_rows, const float* gram, const float* lambda, int nq,
                             int fetch_k, int k, int64_t id_base, const int64_t* id_map, float* out_scores, int64_t* out_ids,
                             int32_t* out_rank, hipStream_t stream);

// ---- bf16 candidate scan + exact re-rank (scan_bf16.hip)
struct ScanBf16Args {
    const unsigned short* corpus;   // tile16b bf16 slab
    const int32_t* row_tag;
    const unsigned short* q_bf16;   // [16*NT][row_stride] normalised queries as bf16
    const int32_t* q_filter;
    float* part_scores;             // [grid][nq][k]
    int64_t* part_ids;              // [grid][nq][k]  LOCAL rows
    int64_t row_stride;             // elements, multiple of 256
    int n_rows;
    int nq;
    int k;                          // candidates kept per query (<= 32)
    int64_t id_base = 0;            // added to the reported rows (0 for the prefilter's candidate scan)
    // EXT variant (as ScanArgs): masked tag compare and the continuation bound of a k > 32 pass
    const int32_t* q_filter_mask = nullptr;
    const float* q_after_score = nullptr;
    const int64_t* q_after_id = nullptr;
    // IVF probe plan over a bf16 slab (all nullptr for the flat scan; as ScanArgs, in 64-row tiles): work item i = slab
    // tile work_tile[i] with work_rows[i] valid rows, visible to the queries whose bit is set in work_mask[i]
    const int32_t* work_tile = nullptr;
    const int32_t* work_rows = nullptr;
    const uint32_t* work_mask = nullptr;
    const int32_t* n_work = nullptr;
    // the sample floor of the flat scan (as ScanI8Args): part_scores [sample_groups][nq][1] of a SAMPLE launch — this kernel with
    // k = 1 over the slab's first 64 * sample_groups rows, same queries and filters; nullptr = none
    const float* sample_best = nullptr;
    int sample_groups = 0;
};
hipError_t launch_scan_bf16_topk(const ScanBf16Args& a, int grid, hipStream_t stream);
// fp32 tile16 blocks -> bf16 tile16b blocks [block0, block1) of dst.  src_block0 (default = block0): the source
// block that lands in block0 (a staging slab); only destination rows in [row_lo, row_hi) are written.
hipError_t launch_convert_tile16_bf16(const float* src, void* dst, int64_t stride, int64_t block0, int64_t block1,
                                      hipStream_t stream, int64_t src_block0 = -1, int64_t row_lo = 0,
                                      int64_t row_hi = -1);
hipError_t launch_unpack_rows_tile16b(const void* slab, int64_t stride, int64_t first_row, int64_t n, int dim,
                                      float* out, int64_t out_stride, hipStream_t stream);
hipError_t launch_queries_to_bf16(const float* src, void* dst, int64_t n, hipStream_t stream);
// The sample floor of a fused fp32 batch, chosen by bf16 MFMAs and scored exactly (sample_rep.hip): the slab's first 64 * grid
// rows, all present, in 32 blocks of 2 * grid; per query and block the eligible row (tag != -1, q_filter < 0 or == tag) with
// the largest bf16 score, lowest row on ties, goes to rep_row[nq][32] (-1: none) and its flat-kernel score to
// sample_best[nq / 32][32][kMaxSampleGroups], entries 0..31 (-inf: none, or not finite).  nq: a multiple of 32; q_padded
// [nq][stride] normalised; scratch: q_frag nq * stride * 2 bytes, rep_part nq * grid * 8 bytes.  Three launches.
bool sample_rep_supported(int64_t stride, int grid);   // stride 128 * {1..8}, grid a multiple of 32 up to kMaxSampleGroups
hipError_t launch_sample_rep(const float* slab, const int32_t* row_tag, int64_t stride, int grid, const float* q_padded,
                             const int32_t* q_filter, int nq, void* q_frag, void* rep_part, int* rep_row, float* sample_best,
                             hipStream_t stream);
// One floor per query, once per batch (sample_rep.hip, step_floors_kernel): floors[q] = what the prologue of a scan selects from
// the first sample_groups entries of sample_best[q][kMaxSampleGroups] — the largest value whose top kFloorBits key bits at least
// k entries reach, -inf when fewer than k entries are above -inf.  q = 0..nq-1, whichever stage filled sample_best.
hipError_t launch_step_floors(const float* sample_best, int sample_groups, int nq, int k, float* floors, hipStream_t stream);
// out_*_group_stride (elements; 0 = contiguous [nq][k]): query q's results go to out + (q / 32) * group_stride + (q % 32) * k
hipError_t launch_rerank_f32(const float* slab, int64_t stride, const float* q_padded, const int64_t* cand_rows, int nq,
                             int n_cand, int k, int64_t id_base, float* out_scores, int64_t* out_ids,
                             hipStream_t stream, int64_t out_scores_group_stride = 0, int64_t out_ids_group_stride = 0,
                             const int64_t* id_map = nullptr);   // id_map: reported id (and tie order) of slab row r = id_map[r]

// ---- int8 candidate scan of the prefilter mode (scan_i8.hip, SURVEY §8f-4 "or int8")
struct ScanI8Args {
    const signed char* corpus;   // tile16i int8 slab
    const float* row_scale;      // [n_rows] max|x| / 127 of every row
    const int32_t* row_tag;      // [n_rows] or nullptr
    const signed char* q_i8;     // [16*NT][row_stride] quantised queries, row-major
    const int32_t* q_filter;     // [nq] or nullptr; -1 = no filter (exact tag compare)
    float* part_scores;          // [grid][nq][k]  (float)(integer dot) * row scale
    int64_t* part_ids;           // [grid][nq][k]  LOCAL rows
    int64_t row_stride;          // bytes per row of the int8 slab: 512 or 1024
    int n_rows;
    int nq;
    int k;                       // candidates kept per query (<= 32)
    // the sample floor (nullptr = none): part_scores [sample_groups][nq][1] of a SAMPLE launch — this kernel with k = 1 over the
    // slab's first 64 * sample_groups rows, same queries and filters; see scan_i8.hip
    const float* sample_best = nullptr;
    int sample_groups = 0;
    const int32_t* q_filter_mask = nullptr;   // [nq] or nullptr: a row matches when (tag & mask) == q_filter
    // grouped launch (flat scans; 0 = off): workgroups [g * wgs_per_group, (g + 1) * wgs_per_group) serve launch group g — its 32
    // queries at q_i8 + g * q_group_stride (bytes), its filters at q_filter + 32 g, its lists at part_scores + g *
    // part_group_stride (elements; part_ids likewise if given).  Every group has nq queries.  Used for the sample launches of a
    // batch call (one launch instead of one per group).
    int wgs_per_group = 0;
    int64_t q_group_stride = 0, part_group_stride = 0;
    // IVF probe plan over an int8 slab (all nullptr for the flat scan; as ScanBf16Args, 64-row tiles)
    const int32_t* work_tile = nullptr;
    const int32_t* work_rows = nullptr;
    const uint32_t* work_mask = nullptr;
    const int32_t* n_work = nullptr;
};
hipError_t launch_scan_i8_topk(const ScanI8Args& a, int grid, hipStream_t stream);
// fp32 tile16 blocks [block0, block1) -> tile16i blocks of dst (+ one scale per row).  stats (nullptr = none): the certified
// mode's per-index maxima [R, V, Y] as float bits, raised by atomicMax with every quantised row's rho, nu and |y| (rounded up)
hipError_t launch_quantize_tile16_i8(const float* src, void* dst, float* scale, int64_t stride, int64_t stride_i8, int64_t block0,
                                     int64_t block1, hipStream_t stream, unsigned* stats = nullptr);

// ---- certified int8 search (prefilter mode 3, scan_i8.hip + certify.hip; DESIGN.md §3 "certified int8 search")
constexpr int kCertQ = 16;        // queries per candidate pass (hi + lo = 32 MFMA columns)
constexpr int kCertC = 128;       // candidates per query
constexpr int kCertWgCap = 256;   // candidate slots per (workgroup, query) of the scan
constexpr int kMaxGridSel = 1024;    // scan workgroups (slices) the selection takes
constexpr int kCertSelCap = 16384;  // candidates per query the selection takes (more: the query is not certified)
struct CertQInfo {                // one query of a pass (queries_to_i8_hilo)
    float s_hi, s_lo;             // q ~ s_hi q_hi + s_lo q_lo
    double qnorm, rho, qa;        // upper bounds of |q|, |q - s_hi q_hi - s_lo q_lo|, |s_hi q_hi| + |s_lo q_lo|
};
struct ScanI8CertArgs {
    const signed char* corpus;    // tile16i slab
    const float* row_scale;
    const int32_t* row_tag;       // or nullptr
    const signed char* q_i8;      // [32][row_stride]: rows 0..15 q_hi, rows 16..31 q_lo
    const CertQInfo* qinfo;       // [16]
    const int32_t* q_filter;      // [nq] or nullptr
    const int32_t* q_filter_mask; // [nq] or nullptr
    int64_t row_stride;
    int n_rows;
    int nq;                       // <= 16
    float* sample_out;            // non-null: a SAMPLE launch — [grid][16] best candidate score per workgroup, nothing else
    const float* sample_best;     // the floor: the floor_rank-th largest of sample_best[0 .. sample_groups)[q]; nullptr = none
    int sample_groups = 0;
    int floor_rank = kCertC;
    float* list_s;                // [grid][16][kCertWgCap] candidate scores (unsorted)
    int32_t* list_r;              // [grid][16][kCertWgCap] their rows
    int32_t* list_n;              // [grid][16] candidates found (may exceed kCertWgCap: overflow)
    float* list_floor;            // [grid][16] the floor if it dropped an eligible row of this workgroup, else -inf
};
hipError_t launch_scan_i8_cert(const ScanI8CertArgs& a, int grid, hipStream_t stream);
hipError_t launch_queries_to_i8_hilo(const float* q_padded, signed char* q_i8, CertQInfo* info, int64_t stride, int64_t stride_i8,
                                     hipStream_t stream);
// per query: the kCertC best (score desc, row asc) of the scan's lists -> cand_rows [4][16][32] (the re-rank's input, -1 past
// the end), optionally cand_s / cand_r [nq][kCertC] (sorted), and tau[q] (certify.hip)
hipError_t launch_cert_select(const float* list_s, const int32_t* list_r, const int32_t* list_n, const float* list_floor, int grid,
                              int nq, int64_t* cand_rows, float* cand_s, int64_t* cand_r, float* tau, hipStream_t stream);
struct CertFinishArgs {
    const float* rr_s;            // [4][16][32] exact scores of the four re-ranked candidate chunks
    const int64_t* rr_i;          // [4][16][32] their reported ids (-1: none)
    const float* tau;             // [nq]
    const CertQInfo* qinfo;
    const unsigned* stats;        // [R, V, Y] float bits
    int dim, nq, k;
    float* out_s;                 // [nq][k]
    int64_t* out_i;
    int32_t* certified;           // [nq] or nullptr
    int32_t* fail_flag;           // [16] 1 = the certificate failed
    int32_t* fail_idx;            // [16] failed queries, compacted
    int32_t* fail_n;              // device scalar
    const float* q_raw;           // [nq][dim] the caller's queries
    const int32_t* q_filter;      // or nullptr
    const int32_t* q_filter_mask; // or nullptr
    float* fb_q;                  // [16][dim] the failed queries, compacted (zero rows after them)
    int32_t* fb_filter;           // [16]
    int32_t* fb_mask;             // [16]
    unsigned long long* counters; // [queries, certified, fallbacks]
};
hipError_t launch_cert_finish(const CertFinishArgs& a, hipStream_t stream);
hipError_t launch_cert_scatter(const float* fb_s, const int64_t* fb_i, const int32_t* fail_idx, const int32_t* fail_n, int k,
                               float* out_s, int64_t* out_i, hipStream_t stream);
hipError_t launch_queries_to_i8(const float* src, void* dst, int nq_pad, int64_t stride, int64_t stride_i8, hipStream_t stream);

// ---- peer-store exchange of per-shard top-k (peer.hip)
hipError_t launch_peer_post(const void* local, size_t bytes, void* remote_slot, void* remote_flag, uint64_t seq,
                            hipStream_t stream);
hipError_t launch_peer_wait(const void* flags, int n, int flag_stride_bytes, uint64_t seq, int* status,
                            int64_t max_spins, hipStream_t stream);

// ---- k-means of the IVF build (kmeans.hip)
struct AssignArgs {
    const float* rows;       // tile16 slab holding the rows to assign (normalised)
    const float* centroids;  // tile16 slab of nlist normalised centroids (whole 16-row blocks)
    int32_t* assign;         // [n_blocks * 32] list of row (b, r) at b*32 + r (compact over the processed blocks)
    float* best;             // optional [n_blocks * 32]: the winning cosine
    int64_t row_stride;      // elements, 128 * {1..8}
    int64_t slab_rows;       // rows ALLOCATED in `rows` (multiple of 16): halves past it read as zero
    int64_t first_block;     // first 32-row block processed ...
    int64_t block_step;      // ... and the stride between processed blocks (a strided training sample)
    int n_blocks;
    int nlist;
};
hipError_t launch_kmeans_assign_f32(const AssignArgs& a, int n_cus, hipStream_t stream);
// sums[assign][0..dim) += row, counts[assign] += 1 over the processed blocks; rows >= n_valid are skipped
hipError_t launch_kmeans_accumulate(const float* rows, int64_t stride, int64_t first_block, int64_t block_step,
                                    int n_blocks, int64_t n_valid, const int32_t* assign, float* sums, float* counts,
                                    int dim, int nlist, hipStream_t stream);

// ---- IVF (ivf.hip)
// Dynamic LDS of the plan kernels, in one place for the launchers and the host code that chooses between them: [nlist] query
// masks + [1 024] scan scratch, and for the batched plan (n_clists > 0) the scores and ids of the 32 queries' n_clists * nprobe
// coarse candidates.  A workgroup gets at most kPlanMaxLdsBytes, the LDS of one CU: the plain plan fits at every nlist the IVF
// takes (135 168 bytes at 32 768), the batched plan with 256 candidates only up to nlist 23 552 (200 704 bytes at 32 768).
constexpr size_t kPlanMaxLdsBytes = 160 * 1024;
constexpr size_t plan_lds_bytes(int nlist, int n_clists, int nprobe) {
    return ((size_t)nlist + 1024 + 2 * 32 * (size_t)n_clists * (size_t)nprobe) * 4;
}
hipError_t launch_plan_probe(const int64_t* probe_ids, int nq, int nprobe, int nlist, const int32_t* list_tile0,
                             const int32_t* list_len, int32_t* work_tile, int32_t* work_rows, uint32_t* work_mask,
                             int32_t* n_work, int64_t* scanned_rows, hipStream_t stream,
                             const uint32_t* preset_mask = nullptr, int tile_rows = 32);
// The plan of a whole batch of launch groups straight from the grouped coarse scan's per-workgroup lists (ivf.hip).
hipError_t launch_plan_probe_groups(const float* cpart_scores, const int64_t* cpart_ids, int n_clists, int nprobe, int groups,
                                    int nq_total, int64_t cpart_group_stride, int nlist, const int32_t* list_tile0,
                                    const int32_t* list_len, int32_t* work_tile, int32_t* work_rows, uint32_t* work_mask,
                                    int64_t work_cap, int32_t* n_work, int64_t* scanned_rows, hipStream_t stream,
                                    int tile_rows);
hipError_t launch_ivf_threshold(const float* part_scores, const int64_t* part_ids, int n_ctiles, int nq, int nprobe,
                                uint32_t* tau_key, hipStream_t stream);
hipError_t launch_ivf_mask_from_scores(const float* part_scores, const int64_t* part_ids, int n_ctiles, int nq,
                                       int nlist, const uint32_t* tau_key, uint32_t* mask, hipStream_t stream);
hipError_t launch_permute_rows_tile16(const float* src, float* dst, int64_t stride, const int64_t* src_of,
                                      int64_t dst_rows, hipStream_t stream);
// the same rows rounded to bf16 into a tile16b slab (the IVF over a bf16 slab)
hipError_t launch_permute_rows_tile16_bf16(const float* src, void* dst, int64_t stride, const int64_t* src_of,
                                           int64_t dst_rows, hipStream_t stream);

// out[r][0..dim) = in[r] / (||in[r]|| + 1e-9); out[r][dim..out_stride) = 0 for r < n;
// rows [n, n_total) of out are zero-filled (query padding), all in one launch.
hipError_t launch_normalize_rows_f32(const float* in, int64_t in_stride, float* out, int64_t out_stride,
                                     int64_t n, int dim, hipStream_t stream, int64_t n_total = 0);

// Zero `n_pad_rows` rows of `stride` floats starting at `dst` (query padding).
hipError_t launch_zero_rows(float* dst, int64_t stride, int n_rows, hipStream_t stream);

// ---- "tile16" corpus layout (what the scan kernel streams) ---------------------------------
// Rows live in 16-row blocks of 16*stride floats.  Inside block b, chunk j (columns
// 16j..16j+15) of the 16 rows is ONE contiguous 1 KiB in MFMA lane order:
//   element (row r, col c) -> (r>>4)*16*stride + (c>>4)*256 + ((((c>>2)&3)*16 + (r&15))*4) + (c&3)
// so a wave's `base + lane*16 B` load is fully coalesced AND already is the A operand of
// v_mfma_f32_16x16x4_f32 (lane = g*16 + m holds row m, k-group g).  A slab holds whole blocks.
inline int64_t tile16_offset(int64_t row, int64_t col, int64_t stride) {
    return (row >> 4) * 16 * stride + (col >> 4) * 256 + ((((col >> 2) & 3) * 16 + (row & 15)) * 4) + (col & 3);
}

// packed rows [first_row, first_row+n) <- in[0..n) row-major; optional reference normalise.
hipError_t launch_pack_rows_tile16(const float* in, int64_t in_stride, float* packed, int64_t stride,
                                   int64_t first_row, int64_t n, int dim, int normalize, hipStream_t stream);
// out[0..n) row-major <- packed rows [first_row, first_row+n).
hipError_t launch_unpack_rows_tile16(const float* packed, int64_t stride, int64_t first_row, int64_t n, int dim,
                                     float* out, int64_t out_stride, hipStream_t stream);
// out[i] <- row row_ids[i] (device array) of the packed slab; ids outside [0, n_rows) leave their output row untouched
hipError_t launch_gather_rows_tile16(const float* packed, int64_t stride, const int64_t* row_ids, int64_t n, int64_t n_rows,
                                     int dim, float* out, int64_t out_stride, hipStream_t stream);

// Synthetic corpus: packed rows [first_row, first_row+n) get iid N(0,1) from Philox4x32-10
// keyed by (seed, row_id_base + row, col/4), L2-normalised; padding columns zero.
hipError_t launch_fill_synthetic_f32(float* packed, int64_t stride, int64_t first_row, int64_t n, int dim,
                                     uint64_t seed, int64_t row_id_base, hipStream_t stream);

// ---- compaction (compact.hip): tombstoned rows squeezed out of a slab, rows only moved
// tags[n_rows] -> new_row[n_rows] (exclusive prefix count of the live rows, -1 for a tombstone), src_row[>= n_live] (its
// inverse) and *n_live, all on the device; three launches, no workgroup waits on another.  workspace: compact_plan_workspace_bytes.
size_t compact_plan_workspace_bytes(int64_t n_rows);
hipError_t launch_compact_plan(const int32_t* tags, int64_t n_rows, int64_t* new_row, int64_t* src_row, int64_t* n_live,
                               void* workspace, hipStream_t stream);
// dst rows [0, n_dst) <- rows src_row[0 .. n_dst) of src, 16 bytes per lane, whole 1 KiB chunks per store; the rows of dst's
// last block past n_dst are zeroed.  tile16 (fp32) and tile16b (bf16): one kernel body, two instantiations.
hipError_t launch_compact_rows_tile16(const float* src, float* dst, int64_t row_stride, const int64_t* src_row, int64_t n_dst,
                                      int64_t n_src_rows, hipStream_t stream);
hipError_t launch_compact_rows_tile16b(const void* src, void* dst, int64_t row_stride, const int64_t* src_row, int64_t n_dst,
                                       int64_t n_src_rows, hipStream_t stream);
// dst[i] = src[src_row[i]], i < n (row tags, reported ids)
hipError_t launch_gather_i32(const int32_t* src, int32_t* dst, const int64_t* src_row, int64_t n, int64_t n_src, hipStream_t stream);
hipError_t launch_gather_i64(const int64_t* src, int64_t* dst, const int64_t* src_row, int64_t n, int64_t n_src, hipStream_t stream);

// ---- the list plan of an IVF build (ivf_build.hip): a stable counting sort of the source rows by list id, rows tagged
// RASS_ROW_TAG_DELETED left out; the outputs are those of rass_ivf_build_prefix's host loops.  Two phases so that a builder
// can size its slab in between; no workgroup waits on another.  workspace: ivf_plan_workspace_bytes(n_rows, nlist), the same
// block for both phases.
// count: list_len[nlist], list_tile0[nlist], *total_tiles (0 for no live row), *n_live (nullptr = not wanted: the sum of
// list_len); *status |= 1 for a live row whose list id is outside [0, nlist), |= 2 when total_tiles * tile_rows exceeds the
// slab limit 0x7fffffc0.
size_t ivf_plan_workspace_bytes(int64_t n_rows, int nlist);
hipError_t launch_ivf_plan_count(const int32_t* assign, const int32_t* tags, int64_t n_rows, int nlist, int tile_rows,
                                 int32_t* list_len, int32_t* list_tile0, int64_t* total_tiles, int64_t* n_live, int32_t* status,
                                 void* workspace, hipStream_t stream);
// place: slab_ids[0 .. max(*total_tiles, 1) * tile_rows) (ascending source row inside a list, -1 on padding) and
// pos_of[n_rows] (-1 for a row in no list).  Nothing is written at or past slab_ids_capacity: *status |= 4 instead.
hipError_t launch_ivf_plan_place(const int32_t* assign, const int32_t* tags, int64_t n_rows, int nlist, int tile_rows,
                                 const int32_t* list_tile0, const int64_t* total_tiles, int64_t* slab_ids,
                                 int64_t slab_ids_capacity, int32_t* pos_of, int32_t* status, void* workspace,
                                 hipStream_t stream);
// assign[slab_ids[p]] = l for every occupied position p of list l (ids outside [0, n_assign) are skipped)
hipError_t launch_ivf_lists_to_assign(const int32_t* list_tile0, const int32_t* list_len, int nlist, int tile_rows,
                                      const int64_t* slab_ids, int64_t slab_rows, int32_t* assign, int64_t n_assign,
                                      hipStream_t stream);

hipError_t launch_fill_i32(int32_t* dst, int64_t n, int32_t value, hipStream_t stream);
// dst[i] = base + i
hipError_t launch_iota_i64(int64_t* dst, int64_t n, int64_t base, hipStream_t stream);
// dst[i] = max(src[i], 0): device-source row tags (negative = reserved tombstone code -> 0)
hipError_t launch_copy_tags_clamped(int32_t* dst, const int32_t* src, int64_t n, hipStream_t stream);

}  // namespace rass
