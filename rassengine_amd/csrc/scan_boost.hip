// scan_boost.hip — the boosted scan: exact top-k of  fused = boost[q] * T(cos) + bonus[q][row]  over a flat fp32 index
// (api_boost.hip, rass_index_search_boosted).  The one scan that ranks by something other than the cosine itself: a dense
// fp32 bonus column in HBM, per query or shared, carries whatever the should-clauses of a hybrid query are worth per row.
//
// scan_boost_f32_kernel<CH, NT> is scan_topk_f32_kernel's flat loop (scan_topk.hip) as scan_flat.h restates it from the blocks
// of scan_core.h: the K axis split over the 8 waves, two 16-row blocks of a tile against NT N-tiles of queries, one
// v_mfma_f32_16x16x4_f32 chain per (row, query) in k order from zero, the partials summed p0 + ... + p7 out of LDS, two
// tiles per barrier, the previous pair ranked between the MFMA chunks of the next — so the cosine s is that kernel's bit
// for bit.  The ranking then computes, as separately rounded fp32 operations (the Makefile turns contraction off for this
// object),
//     t = s                      (transform 0)
//     t = 1.0f / (2.0f - s)      (transform 1: the reference's score mode; correctly rounded division, hipcc's default)
//     fused = boost[q] * t + b
// and inserts fused.  A row ranks for query q when it is live, passes q's masked filter, lies strictly after q's
// continuation bound on the FUSED score, has s > -inf (a NaN or -inf cosine never ranks, whatever the bonus) and has
// fused > -inf (a NaN or -inf bonus excludes the row: that is how a bitmap composes, bonus_mask_kernel in bonus.hip).
// No sample floor: a floor is only valid under the score it was sampled with.
//
// Where the bonus lives: the lane that ranks a (row, query) fetches its own value a tile pair ahead of the corpus refills and
// parks it in LDS where the pair is ranked one iteration later (scan_flat.h, PairColumn, says why).  A lane whose row is at
// or past bonus_rows (rows appended after the column was built), past the tile's rows, or in a run-ahead tile gets an offset
// past the records: 0 comes back and no memory request is made.
//
// Plain vector loads and stores only.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "scan_flat.h"

namespace rass {

template <int NT>
struct BoostPolicy {
    const BoostArgs& b;
    AfterBound after;
    float* boost;            // LDS [32]
    PairColumn<NT, true> col;
    TopList L[NT];

    __device__ __forceinline__ void setup(int q, bool live) {
        after.setup(b.scan, q, live);
        boost[q] = (b.boost != nullptr && live) ? b.boost[q] : 1.0f;
    }
    // the rows of a tile that have a bonus: none at or past bonus_rows
    __device__ __forceinline__ int bonus_rows_of(const WorkItem& w) const {
        const int64_t left = b.bonus_rows - (int64_t)w.tile * kTileRows;
        return left < (int64_t)w.rows ? (left < 0 ? 0 : (int)left) : w.rows;
    }
    __device__ __forceinline__ void pair_top(const WorkItem& w0, const WorkItem& w1) {
        col.park_and_request(w0.tile, bonus_rows_of(w0), w1.tile, bonus_rows_of(w1));
    }
    __device__ __forceinline__ void tile_ahead(int, const WorkItem&) {}
    __device__ __forceinline__ void last_pair() { col.park(); }
    // The fused score of one (row, query), inserted into the query's list.
    __device__ __forceinline__ void rank(const FlatPart<NT>& c, int, int which, int pq) {
        const float bon = col.parked[which][pq][c.tid];
        const float s = c.score();
        float tr = s;
        if (b.transform) tr = 1.0f / (2.0f - s);   // a kernel argument: a scalar branch
        float fused = __fadd_rn(__fmul_rn(boost[c.q], tr), bon);
        // NaN and -inf never rank (include/rass_engine.h, "Scores that are not finite"): not as a cosine, not as a fused score
        const float as = after.s[c.q];
        const bool live = c.live();
        const bool ok = live & (s > -INFINITY) & (fused > -INFINITY) & after.passes(c.q, as, fused, c.row);
        fused = ok ? fused : -INFINITY;
        float tau = bcast_kth(L[pq].s, b.scan.k);
        insert_candidates(L[pq], tau, fused, c.row, b.scan.k);
    }
};

template <int CH, int NT>
__global__ __launch_bounds__(kThreads, 2) void scan_boost_f32_kernel(BoostArgs b) {
    __shared__ int sh_qfilt[32];
    __shared__ int sh_qmask[32];
    __shared__ float sh_after_s[32];
    __shared__ int64_t sh_after_i[32];
    __shared__ float sh_boost[32];
    __shared__ int sh_tags[4][32];
    __shared__ float sh_bonus[2][NT][kThreads];
    BoostPolicy<NT> pol{b, {sh_after_s, sh_after_i}, sh_boost};
    init_lists(pol.L);
    pol.col.setup(b.bonus, b.bonus_bytes, b.bonus_q_stride, b.scan.nq, sh_bonus);
    flat_pair_scan<CH, NT>(b.scan, FlatShared{sh_qfilt, sh_qmask, sh_tags}, pol);
    store_lists(b.scan, pol.L);
}

struct BoostFamily {
    template <int CH, int NT>
    static constexpr auto kernel() { return &scan_boost_f32_kernel<CH, NT>; }
};

hipError_t launch_scan_boost_f32(const BoostArgs& a, int grid, hipStream_t stream) {
    const ScanArgs& s = a.scan;
    if (!flat_scan_args_ok(s, grid)) return hipErrorInvalidValue;
    if (s.k < 1 || s.k > 32 || !s.part_scores || !s.part_ids || !a.bonus) return hipErrorInvalidValue;
    if ((s.q_after_score == nullptr) != (s.q_after_id == nullptr)) return hipErrorInvalidValue;
    if (s.allow || s.group_table) return hipErrorInvalidValue;
    // every in-range lane's offset lies inside the descriptor: (nq - 1) columns of bonus_q_stride, then bonus_rows values
    if (a.bonus_rows < 0 || a.bonus_q_stride < 0 || (a.bonus_q_stride > 0 && a.bonus_rows > a.bonus_q_stride)) return hipErrorInvalidValue;
    const int64_t need = ((int64_t)(a.bonus_q_stride > 0 ? s.nq - 1 : 0) * a.bonus_q_stride + a.bonus_rows) * 4;
    if (need > kBoostMaxBonusBytes || (int64_t)a.bonus_bytes != need) return hipErrorInvalidValue;
    if (a.transform != 0 && a.transform != 1) return hipErrorInvalidValue;
    return launch_flat_family<BoostFamily>(a, grid, stream);
}

}  // namespace rass
