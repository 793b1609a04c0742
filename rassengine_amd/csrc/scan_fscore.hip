// scan_fscore.hip — the function-score scan: exact top-k of  fused = combine(boost[q] * T(cos), fn[q][row])  over a flat fp32
// index (rass_index_search_scored: entry points in api_fscore.hip, search path in api_boost.hip), with a per-query gate on the
// transformed similarity.  OpenSearch's function_score around a k-NN clause: the function column (score_fn.hip builds it from
// decay, field-value and weight functions) is combined with the similarity by any boost_mode, not only summed as the boosted
// scan does.
//
// scan_fscore_f32_kernel<CH, NT> runs the loop the boosted scan runs (scan_flat.h), a family and an object of its own so
// that the boosted family keeps its kernels and its resource use: the same blocks of scan_core.h, the K axis split over the
// 8 waves, one v_mfma_f32_16x16x4_f32 chain per (row, query) in k order from zero, the partials summed p0 + ... + p7 out of
// LDS, two tiles per barrier, the previous pair ranked between the MFMA chunks of the next — so the cosine s is the flat
// scan's bit for bit.  The ranking then computes, as separately rounded fp32 operations (the Makefile turns contraction off
// for this object),
//     t = s                      (transform 0)
//     t = 1.0f / (2.0f - s)      (transform 1; correctly rounded division, hipcc's default)
//     a = boost[q] * t
//     fused = a + f | a * f | (a + f) * 0.5f | f > a ? f : a | f < a ? f : a | f        (mode 0 .. 5, a kernel argument;
//                                                                                        all computed, one selected)
// max and min are a compare and a select: fmaxf / fminf leave the sign of a zero open, and scores are compared bit for bit.
// A row ranks for query q when it is live, passes q's masked filter, lies strictly after q's continuation bound on the FUSED
// score, has s > -inf, has fused > -inf, has t >= gate[q] (the k-NN clause's radial min_score; -inf: no gate) and has
// f > -inf: a NaN or -inf cell of the column excludes the row in every mode, max and replace included, which keeps
// bonus_mask_kernel (bonus.hip) usable on a function column.  No sample floor.
//
// The column is fetched as the boosted scan fetches its bonus (scan_flat.h, PairColumn): the lane that ranks a (row, query)
// requests its own value a tile pair ahead of the corpus refills, through one buffer descriptor, and parks it in LDS ([2
// tiles][NT][512 threads] floats) where the pair is ranked one iteration later — no wait drains the corpus stream, and 2 * NT
// VGPRs live across the loop.  The column covers every row of the slab (launch_scan_fscore_f32 checks fn_rows == n_rows); a
// lane past the tile's rows or in a run-ahead tile gets an offset past the records: 0 comes back, no memory request is made,
// and the row does not rank because it does not exist.
//
// Plain vector loads and stores only.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "scan_flat.h"

namespace rass {

template <int NT>
struct FscorePolicy {
    const FscoreArgs& b;
    AfterBound after;
    float* boost;            // LDS [32]
    float* gate;             // LDS [32]
    PairColumn<NT, false> col;
    TopList L[NT];

    __device__ __forceinline__ void setup(int q, bool live) {
        after.setup(b.scan, q, live);
        boost[q] = (b.boost != nullptr && live) ? b.boost[q] : 1.0f;
        gate[q] = (b.min_score != nullptr && live) ? b.min_score[q] : -INFINITY;
    }
    __device__ __forceinline__ void pair_top(const WorkItem& w0, const WorkItem& w1) {
        col.park_and_request(w0.tile, w0.rows, w1.tile, w1.rows);
    }
    __device__ __forceinline__ void tile_ahead(int, const WorkItem&) {}
    __device__ __forceinline__ void last_pair() { col.park(); }
    // The fused score of one (row, query), inserted into the query's list.
    __device__ __forceinline__ void rank(const FlatPart<NT>& c, int, int which, int pq) {
        const float f = col.parked[which][pq][c.tid];
        const float s = c.score();
        float tr = s;
        if (b.transform) tr = 1.0f / (2.0f - s);   // a kernel argument: a scalar branch
        const float a = __fmul_rn(boost[c.q], tr);
        // every mode's value, then selects on the mode (a kernel argument: the conditions are wave-uniform).  No branch: the
        // ranking step is scheduled between the MFMA chunks, and a six-way scalar branch there cost 1 - 2 % of the launch
        // group (measured).  The operations whose result is not taken are rounded and dropped.
        const float sum = __fadd_rn(a, f);
        float fused = sum;
        fused = b.mode == 1 ? __fmul_rn(a, f) : fused;
        fused = b.mode == 2 ? __fmul_rn(sum, 0.5f) : fused;
        fused = b.mode == 3 ? (f > a ? f : a) : fused;
        fused = b.mode == 4 ? (f < a ? f : a) : fused;
        fused = b.mode == 5 ? f : fused;
        // NaN and -inf never rank (include/rass_engine.h, "Scores that are not finite"): not as a cosine, not as a column cell,
        // not as a fused score; a NaN t fails the gate
        const float as = after.s[c.q];
        const bool live = c.live();
        const bool ok = live & (s > -INFINITY) & (f > -INFINITY) & (tr >= gate[c.q]) & (fused > -INFINITY) &
                        after.passes(c.q, as, fused, c.row);
        fused = ok ? fused : -INFINITY;
        float tau = bcast_kth(L[pq].s, b.scan.k);
        insert_candidates(L[pq], tau, fused, c.row, b.scan.k);
    }
};

template <int CH, int NT>
__global__ __launch_bounds__(kThreads, 2) void scan_fscore_f32_kernel(FscoreArgs b) {
    __shared__ int sh_qfilt[32];
    __shared__ int sh_qmask[32];
    __shared__ float sh_after_s[32];
    __shared__ int64_t sh_after_i[32];
    __shared__ float sh_boost[32];
    __shared__ float sh_gate[32];
    __shared__ int sh_tags[4][32];
    __shared__ float sh_fn[2][NT][kThreads];
    FscorePolicy<NT> pol{b, {sh_after_s, sh_after_i}, sh_boost, sh_gate};
    init_lists(pol.L);
    pol.col.setup(b.fn, b.fn_bytes, b.fn_q_stride, b.scan.nq, sh_fn);
    flat_pair_scan<CH, NT>(b.scan, FlatShared{sh_qfilt, sh_qmask, sh_tags}, pol);
    store_lists(b.scan, pol.L);
}

struct FscoreFamily {
    template <int CH, int NT>
    static constexpr auto kernel() { return &scan_fscore_f32_kernel<CH, NT>; }
};

hipError_t launch_scan_fscore_f32(const FscoreArgs& a, int grid, hipStream_t stream) {
    const ScanArgs& s = a.scan;
    if (!flat_scan_args_ok(s, grid)) return hipErrorInvalidValue;
    if (s.k < 1 || s.k > 32 || !s.part_scores || !s.part_ids || !a.fn) return hipErrorInvalidValue;
    if ((s.q_after_score == nullptr) != (s.q_after_id == nullptr)) return hipErrorInvalidValue;
    if (s.allow || s.group_table) return hipErrorInvalidValue;
    // the column covers exactly the slab's rows, and every in-range lane's offset lies inside the descriptor: (nq - 1)
    // columns of fn_q_stride, then fn_rows values
    if (a.fn_rows != (int64_t)s.n_rows || a.fn_q_stride < 0 || (a.fn_q_stride > 0 && a.fn_rows > a.fn_q_stride)) return hipErrorInvalidValue;
    const int64_t need = ((int64_t)(a.fn_q_stride > 0 ? s.nq - 1 : 0) * a.fn_q_stride + a.fn_rows) * 4;
    if (need > kBoostMaxBonusBytes || (int64_t)a.fn_bytes != need) return hipErrorInvalidValue;
    if (a.transform != 0 && a.transform != 1) return hipErrorInvalidValue;
    if (a.mode < 0 || a.mode >= kCombineModes) return hipErrorInvalidValue;
    return launch_flat_family<FscoreFamily>(a, grid, stream);
}

}  // namespace rass
