// scan_fscore.hip — the function-score scan: exact top-k of  fused = combine(boost[q] * T(cos), fn[q][row])  over a flat fp32
// index (api_fscore.hip, rass_index_search_scored), with a per-query gate on the transformed similarity.  OpenSearch's
// function_score around a k-NN clause: the function column (score_fn.hip builds it from decay, field-value and weight
// functions) is combined with the similarity by any boost_mode, not only summed as the boosted scan does.
//
// scan_fscore_f32_kernel<CH, NT> is scan_boost_f32_kernel's loop (scan_boost.hip) restated, a family and an object of its own
// so that the boosted family keeps its kernels and its resource use: the same blocks of scan_core.h, the K axis split over the
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
// The column is fetched as the boosted scan fetches its bonus: the lane that ranks a (row, query) requests its own value a
// tile pair ahead of the corpus refills, through one buffer descriptor, and parks it in LDS ([2 tiles][NT][512 threads]
// floats) where the pair is ranked one iteration later — no wait drains the corpus stream, and 2 * NT VGPRs live across the
// loop.  The column covers every row of the slab (launch_scan_fscore_f32 checks fn_rows == n_rows); a lane past the tile's
// rows or in a run-ahead tile gets an offset past the records: 0 comes back, no memory request is made, and the row does not
// rank because it does not exist.
//
// Plain vector loads and stores only.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "scan_core.h"

namespace rass {

template <int CH, int NT>
__global__ __launch_bounds__(kThreads, 2) void scan_fscore_f32_kernel(FscoreArgs b) {
    const ScanArgs& p = b.scan;
    constexpr int NQ = NT * 16;
    extern __shared__ __attribute__((aligned(16))) float lds[];  // [4][kWaves][NQ][kPitch]

    const int lane = lane_id();
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = lane & 15, g = lane >> 4;
    const int G = gridDim.x, bid = blockIdx.x;
    const int n_tiles = (p.n_rows + kTileRows - 1) / kTileRows;

    // Query fragments: lane (n = m, g) holds Qn[nt*16 + n][slice + 16j + 4g .. +3].
    f32x4 qf[NT][CH];
    {
        const float* qbase = p.q_padded + (int64_t)m * p.row_stride + wid * 16 * CH + 4 * g;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int j = 0; j < CH; ++j)
                qf[nt][j] = *reinterpret_cast<const f32x4*>(qbase + (int64_t)nt * 16 * p.row_stride + 16 * j);
    }
    const int voff_lane = wid * CH * 1024 + lane * 16;

    // Top-k state: pass pq handles query pq*16 + (lane>>5)*8 + wid for row lane&31 (the threshold of a list is re-read from
    // the list at every ranking step, as in the boosted scan)
    TopList L[NT];
#pragma unroll
    for (int pq = 0; pq < NT; ++pq) {
        L[pq].s = -INFINITY;
        L[pq].i = 0x7fffffff;
    }
    __shared__ int sh_qfilt[32];
    __shared__ int sh_qmask[32];
    __shared__ float sh_after_s[32];
    __shared__ int64_t sh_after_i[32];
    __shared__ float sh_boost[32];
    __shared__ float sh_gate[32];
    __shared__ int sh_tags[4][32];
    __shared__ float sh_fn[2][NT][kThreads];   // the pair being ranked: [tile of the pair][pq][thread], lane-private
    if (threadIdx.x < 32) {
        const int q = threadIdx.x;
        const bool live = q < p.nq;
        sh_qfilt[q] = (p.q_filter != nullptr && live) ? p.q_filter[q] : -1;
        sh_qmask[q] = (p.q_filter_mask != nullptr && live) ? p.q_filter_mask[q] : -1;
        sh_after_s[q] = (p.q_after_score != nullptr && live) ? p.q_after_score[q] : INFINITY;
        sh_after_i[q] = (p.q_after_id != nullptr && live) ? p.q_after_id[q] : (int64_t)-1;
        sh_boost[q] = (b.boost != nullptr && live) ? b.boost[q] : 1.0f;
        sh_gate[q] = (b.min_score != nullptr && live) ? b.min_score[q] : -INFINITY;
    }
    __syncthreads();

    // The column value of this lane's (row, query) of a tile.  Queries past nq (zero rows, never written) read the last live
    // query's column: in bounds.  The two halves' column offsets are wave-uniform; one select picks the lane's.
    const __amdgpu_buffer_rsrc_t fn_rsrc = make_rsrc(reinterpret_cast<uint64_t>(b.fn), b.fn_bytes);
    // Per-lane offsets and LDS addresses are derived, where they are used, from a lane id hipcc cannot see through (see
    // scan_boost.hip: left visible they are hoisted and kept live across the tile loop).
    auto hidden = [](int v) {
        asm volatile("" : "+v"(v));
        return v;
    };
    auto load_fn = [&](const WorkItem& w, int pq) {
        const int lane = hidden(lane_id());
        const unsigned r4 = (unsigned)(lane & 31) * 4u;
        const int qa = min(pq * 16 + wid, p.nq - 1), qb = min(pq * 16 + 8 + wid, p.nq - 1);
        const unsigned tile_off = (unsigned)w.tile * (unsigned)(kTileRows * 4);
        const unsigned offa = (unsigned)((int64_t)qa * b.fn_q_stride * 4) + tile_off;
        const unsigned offb = (unsigned)((int64_t)qb * b.fn_q_stride * 4) + tile_off;
        const bool valid = (lane & 31) < w.rows;
        const unsigned voff = valid ? ((lane & 32) ? offb : offa) + r4 : 0xffffffffu;
        return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(fn_rsrc, (int)voff, 0, 0));
    };

    const int mt_step = 16 * (int)p.row_stride * 4;
    TileRegs<CH> R0, R1;
    int t = bid;          // the item R0 holds; R1 holds t + G, then every workgroup steps by 2 G
    auto work = [&](int i) {
        int rows = p.n_rows - i * kTileRows;
        rows = rows < 0 ? 0 : (rows > kTileRows ? kTileRows : rows);
        WorkItem w;
        w.tile = i < n_tiles ? i : 0;
        w.rows = i < n_tiles ? rows : 0;
        w.mask = 0xffffffffu;
        return w;
    };
    WorkItem W0 = work(t), W1 = work(t + G);
    issue_tile_loads<CH>(R0, make_tile_desc(p.corpus, p.row_stride, p.row_tag, W0), voff_lane, mt_step);
    issue_tile_loads<CH>(R1, make_tile_desc(p.corpus, p.row_stride, p.row_tag, W1), voff_lane, mt_step);
    __builtin_amdgcn_sched_barrier(0);

    auto dump_tile = [&](const f32x4 (&acc)[2][NT], int buf) {
        float* P = lds + buf * (kWaves * NQ * kPitch);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                *reinterpret_cast<f32x4*>(P + (wid * NQ + nt * 16 + m) * kPitch + mt * 16 + 4 * g) = acc[mt][nt];
    };
    // Rank one (tile, query group pq) of a dumped tile: the cosine as scan_topk_f32_kernel sums it, then the fused score.
    auto rank_part = [&](const WorkItem& w, int buf, int which, int pq) {
        const int tid = hidden((int)threadIdx.x), lane = tid & 63;
        const float* P = lds + buf * (kWaves * NQ * kPitch);
        const int r = lane & 31;
        const int row = w.tile * kTileRows + r;
        const int tag = sh_tags[buf][r];
        const int q = pq * 16 + (lane >> 5) * 8 + wid;
        const int qf1 = sh_qfilt[q];
        const float f = sh_fn[which][pq][tid];
        const float* src = P + q * kPitch + r;
        float s = src[0];
#pragma unroll
        for (int wv = 1; wv < kWaves; ++wv) s += src[wv * NQ * kPitch];
        float tr = s;
        if (b.transform) tr = 1.0f / (2.0f - s);   // a kernel argument: a scalar branch
        const float a = __fmul_rn(sh_boost[q], tr);
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
        const float as = sh_after_s[q];
        // NaN and -inf never rank (include/rass_engine.h, "Scores that are not finite"): not as a cosine, not as a column cell,
        // not as a fused score; a NaN t fails the gate
        const bool ok = (r < w.rows) & (tag != -1) & ((qf1 < 0) | (qf1 == (tag & sh_qmask[q]))) & (s > -INFINITY) & (f > -INFINITY) &
                        (tr >= sh_gate[q]) & (fused > -INFINITY) & ((fused < as) | ((fused == as) & ((int64_t)row > sh_after_i[q])));
        fused = ok ? fused : -INFINITY;
        float tau = bcast_kth(L[pq].s, p.k);
        insert_candidates(L[pq], tau, fused, row, p.k);
    };

    constexpr int kParts = 2 * NT;
    auto slot_of = [](int part) { return max(((part + 1) * 2 * CH) / kParts - 1, 0); };
    WorkItem Pa{0, 0, 0u}, Pb{0, 0, 0u};  // the previous pair (rows = 0: nothing ranks in the first iteration)
    float FA[NT], FB[NT];                 // the column values of the pair last requested (tile A, tile B)
#pragma unroll
    for (int pq = 0; pq < NT; ++pq) FA[pq] = FB[pq] = 0.f;
    auto park_fn = [&]() {
        const int tid = hidden((int)threadIdx.x);
#pragma unroll
        for (int pq = 0; pq < NT; ++pq) {
            sh_fn[0][pq][tid] = FA[pq];
            sh_fn[1][pq][tid] = FB[pq];
        }
    };
    int pair = 0;  // 0 / 2: which two LDS images this iteration dumps into
    while (t < n_tiles) {
        f32x4 acc[2][NT];
        if (wid == 0 && lane < 32) {
            sh_tags[pair][lane] = R0.tag;
            sh_tags[pair + 1][lane] = R1.tag;
        }
        // the previous pair's values have arrived (requested before the loads whose tags were just stored): park them for
        // this iteration's ranking, then request this pair's, ahead of the refills below
        park_fn();
#pragma unroll
        for (int pq = 0; pq < NT; ++pq) {
            FA[pq] = load_fn(W0, pq);
            FB[pq] = load_fn(W1, pq);
        }
        const WorkItem Wa = W0;
        t += 2 * G;
        WorkItem Wn = work(t);
        auto rank_prev = [&](int slot) {
#pragma unroll
            for (int part = 0; part < kParts; ++part)
                if (slot_of(part) == slot) {
                    if (part < NT)
                        rank_part(Pa, pair ^ 2, 0, part);
                    else
                        rank_part(Pb, (pair ^ 2) + 1, 1, part - NT);
                }
        };
        multiply_and_refill<CH, NT>(R0, qf, acc, make_tile_desc(p.corpus, p.row_stride, p.row_tag, Wn), voff_lane, mt_step,
                                    [&](int j) { rank_prev(j); });
        dump_tile(acc, pair);
        W0 = Wn;
        const WorkItem Wb = W1;
        Wn = work(t + G);
        multiply_and_refill<CH, NT>(R1, qf, acc, make_tile_desc(p.corpus, p.row_stride, p.row_tag, Wn), voff_lane, mt_step,
                                    [&](int j) { rank_prev(CH + j); });
        dump_tile(acc, pair + 1);
        W1 = Wn;
        Pa = Wa;
        Pb = Wb;
        __syncthreads();
        pair ^= 2;
    }
    // the last pair
    park_fn();
#pragma unroll
    for (int pq = 0; pq < NT; ++pq) rank_part(Pa, pair ^ 2, 0, pq);
#pragma unroll
    for (int pq = 0; pq < NT; ++pq) rank_part(Pb, (pair ^ 2) + 1, 1, pq);

    // Per-workgroup sorted lists -> [gridDim.x][nq][k]
    const int lpos = lane & 31;
#pragma unroll
    for (int pq = 0; pq < NT; ++pq) {
        const int q = pq * 16 + (lane >> 5) * 8 + wid;
        if (q < p.nq && lpos < p.k) {
            const int64_t o = ((int64_t)bid * p.nq + q) * p.k + lpos;
            const bool filled = L[pq].i != 0x7fffffff;
            p.part_scores[o] = filled ? L[pq].s : -INFINITY;
            p.part_ids[o] = filled ? (int64_t)L[pq].i : (int64_t)-1;
        }
    }
}

template <int CH, int NT>
static hipError_t launch_fscore_variant(const FscoreArgs& a, int grid, hipStream_t stream) {
    constexpr size_t lds_bytes = (size_t)4 * kWaves * NT * 16 * kPitch * sizeof(float);  // 144 KiB at NT = 2
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&scan_fscore_f32_kernel<CH, NT>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    hipLaunchKernelGGL((scan_fscore_f32_kernel<CH, NT>), dim3(grid), dim3(kThreads), lds_bytes, stream, a);
    return hipGetLastError();
}

template <int NT>
static hipError_t launch_fscore_ch(int ch, const FscoreArgs& a, int grid, hipStream_t stream) {
    switch (ch) {
        case 1: return launch_fscore_variant<1, NT>(a, grid, stream);
        case 2: return launch_fscore_variant<2, NT>(a, grid, stream);
        case 3: return launch_fscore_variant<3, NT>(a, grid, stream);
        case 4: return launch_fscore_variant<4, NT>(a, grid, stream);
        case 5: return launch_fscore_variant<5, NT>(a, grid, stream);
        case 6: return launch_fscore_variant<6, NT>(a, grid, stream);
        case 7: return launch_fscore_variant<7, NT>(a, grid, stream);
        case 8: return launch_fscore_variant<8, NT>(a, grid, stream);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_scan_fscore_f32(const FscoreArgs& a, int grid, hipStream_t stream) {
    const ScanArgs& s = a.scan;
    if (s.row_stride % 128 != 0 || s.row_stride < 128 || s.row_stride > 1024) return hipErrorInvalidValue;   // narrow rows only
    if (s.nq < 1 || s.nq > 32 || s.k < 1 || s.k > 32 || s.n_rows < 1 || grid < 1) return hipErrorInvalidValue;
    if (!s.corpus || !s.q_padded || !s.part_scores || !s.part_ids || !a.fn) return hipErrorInvalidValue;
    if ((s.q_after_score == nullptr) != (s.q_after_id == nullptr)) return hipErrorInvalidValue;
    if (s.q_filter_mask != nullptr && s.q_filter == nullptr) return hipErrorInvalidValue;
    if (s.q_filter != nullptr && s.row_tag == nullptr) return hipErrorInvalidValue;
    if (s.work_tile || s.work_base || s.sample_pass || s.sample_best || s.wgs_per_group || s.live_nq || s.allow || s.range_count ||
        s.group_table || s.count_table || s.id_base != 0)
        return hipErrorInvalidValue;
    // the column covers exactly the slab's rows, and every in-range lane's offset lies inside the descriptor: (nq - 1)
    // columns of fn_q_stride, then fn_rows values
    if (a.fn_rows != (int64_t)s.n_rows || a.fn_q_stride < 0 || (a.fn_q_stride > 0 && a.fn_rows > a.fn_q_stride)) return hipErrorInvalidValue;
    const int64_t need = ((int64_t)(a.fn_q_stride > 0 ? s.nq - 1 : 0) * a.fn_q_stride + a.fn_rows) * 4;
    if (need > kBoostMaxBonusBytes || (int64_t)a.fn_bytes != need) return hipErrorInvalidValue;
    if (a.transform != 0 && a.transform != 1) return hipErrorInvalidValue;
    if (a.mode < 0 || a.mode >= kCombineModes) return hipErrorInvalidValue;
    const int ch = (int)(s.row_stride / 128);
    return s.nq <= 16 ? launch_fscore_ch<1>(ch, a, grid, stream) : launch_fscore_ch<2>(ch, a, grid, stream);
}

}  // namespace rass
