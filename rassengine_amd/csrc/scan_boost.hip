// scan_boost.hip — the boosted scan: exact top-k of  fused = boost[q] * T(cos) + bonus[q][row]  over a flat fp32 index
// (api_boost.hip, rass_index_search_boosted).  The one scan that ranks by something other than the cosine itself: a dense
// fp32 bonus column in HBM, per query or shared, carries whatever the should-clauses of a hybrid query are worth per row.
//
// scan_boost_f32_kernel<CH, NT> is scan_topk_f32_kernel's flat loop (scan_topk.hip) built from the same blocks of
// scan_core.h: the K axis split over the 8 waves, two 16-row blocks of a tile against NT N-tiles of queries, one
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
// Where the bonus lives.  Lane (r = lane & 31, half = lane >> 5) of wave w ranks row r of a tile for query pq * 16 + half * 8
// + w, so the lane that ranks a (row, query) can fetch its own bonus: NT coalesced 64-lane loads per tile, two 128-byte
// runs each, and no lane exchange.  Issued inside the ranking step, such a load would make the step wait on vmcnt, which
// counts in order: the wait would drain the two tiles of corpus loads in flight (the trap the KEYS bitmap read of
// scan_topk.hip describes).  So a pair's 2 * NT values are requested at the TOP of the iteration that multiplies the pair,
// ahead of that iteration's refill loads; one iteration later, where the pair is ranked, the wait for the refilled tags
// has seen them come back.  There they are parked in LDS — [2 tiles][NT][512 threads] floats, 8 KiB at NT = 2 beside the
// 144 KiB of partial images, each lane writing and reading its own slot, so no barrier is involved — and the registers take
// the next pair's request: 2 * NT VGPRs live across the loop instead of 4 * NT, which CH = 8 / NT = 2 does not have.
// Each bonus load goes through one buffer descriptor over the launch group's column(s); a lane whose row is at or past
// bonus_rows (rows appended after the column was built), past the tile's rows, or in a run-ahead tile gets an offset past
// the records: 0 comes back and no memory request is made.
//
// Plain vector loads and stores only.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "scan_core.h"

namespace rass {

template <int CH, int NT>
__global__ __launch_bounds__(kThreads, 2) void scan_boost_f32_kernel(BoostArgs b) {
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

    // Top-k state: pass pq handles query pq*16 + (lane>>5)*8 + wid for row lane&31.
    // (the threshold of a list — its k-th score — is re-read from the list at every ranking step, not carried: two readlanes
    // against a register per list that CH = 8 / NT = 2 does not have)
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
    __shared__ int sh_tags[4][32];
    __shared__ float sh_bonus[2][NT][kThreads];   // the pair being ranked: [tile of the pair][pq][thread], lane-private
    if (threadIdx.x < 32) {
        const int q = threadIdx.x;
        const bool live = q < p.nq;
        sh_qfilt[q] = (p.q_filter != nullptr && live) ? p.q_filter[q] : -1;
        sh_qmask[q] = (p.q_filter_mask != nullptr && live) ? p.q_filter_mask[q] : -1;
        sh_after_s[q] = (p.q_after_score != nullptr && live) ? p.q_after_score[q] : INFINITY;
        sh_after_i[q] = (p.q_after_id != nullptr && live) ? p.q_after_id[q] : (int64_t)-1;
        sh_boost[q] = (b.boost != nullptr && live) ? b.boost[q] : 1.0f;
    }
    __syncthreads();

    // The bonus of this lane's (row, query) of a tile.  Queries past nq (zero rows, never written) read the last live
    // query's column: in bounds.  The two halves' column offsets are wave-uniform; one select picks the lane's.
    const __amdgpu_buffer_rsrc_t bonus_rsrc = make_rsrc(reinterpret_cast<uint64_t>(b.bonus), b.bonus_bytes);
    // Per-lane offsets and LDS addresses are derived, where they are used, from a lane id hipcc cannot see through: left visible
    // they are loop invariants, hoisted and kept live across the tile loop, which has no register to spare at CH = 8 / NT = 2.
    auto hidden = [](int v) {
        asm volatile("" : "+v"(v));
        return v;
    };
    auto load_bonus = [&](const WorkItem& w, int pq) {
        const int lane = hidden(lane_id());
        const unsigned r4 = (unsigned)(lane & 31) * 4u;
        const int qa = min(pq * 16 + wid, p.nq - 1), qb = min(pq * 16 + 8 + wid, p.nq - 1);
        const unsigned tile_off = (unsigned)w.tile * (unsigned)(kTileRows * 4);
        const unsigned offa = (unsigned)((int64_t)qa * b.bonus_q_stride * 4) + tile_off;
        const unsigned offb = (unsigned)((int64_t)qb * b.bonus_q_stride * 4) + tile_off;
        const int64_t left = b.bonus_rows - (int64_t)w.tile * kTileRows;
        const int n = left < (int64_t)w.rows ? (left < 0 ? 0 : (int)left) : w.rows;
        const bool valid = (lane & 31) < n;
        const unsigned voff = valid ? ((lane & 32) ? offb : offa) + r4 : 0xffffffffu;
        return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(bonus_rsrc, (int)voff, 0, 0));
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
        const float bon = sh_bonus[which][pq][tid];
        const float* src = P + q * kPitch + r;
        float s = src[0];
#pragma unroll
        for (int wv = 1; wv < kWaves; ++wv) s += src[wv * NQ * kPitch];
        float tr = s;
        if (b.transform) tr = 1.0f / (2.0f - s);   // a kernel argument: a scalar branch
        float fused = __fadd_rn(__fmul_rn(sh_boost[q], tr), bon);
        const float as = sh_after_s[q];
        // NaN and -inf never rank (include/rass_engine.h, "Scores that are not finite"): not as a cosine, not as a fused score
        const bool ok = (r < w.rows) & (tag != -1) & ((qf1 < 0) | (qf1 == (tag & sh_qmask[q]))) & (s > -INFINITY) &
                        (fused > -INFINITY) & ((fused < as) | ((fused == as) & ((int64_t)row > sh_after_i[q])));
        fused = ok ? fused : -INFINITY;
        float tau = bcast_kth(L[pq].s, p.k);
        insert_candidates(L[pq], tau, fused, row, p.k);
    };

    constexpr int kParts = 2 * NT;
    auto slot_of = [](int part) { return max(((part + 1) * 2 * CH) / kParts - 1, 0); };
    WorkItem Pa{0, 0, 0u}, Pb{0, 0, 0u};  // the previous pair (rows = 0: nothing ranks in the first iteration)
    float BA[NT], BB[NT];                 // the bonus of the pair last requested (tile A, tile B)
#pragma unroll
    for (int pq = 0; pq < NT; ++pq) BA[pq] = BB[pq] = 0.f;
    auto park_bonus = [&]() {
        const int tid = hidden((int)threadIdx.x);
#pragma unroll
        for (int pq = 0; pq < NT; ++pq) {
            sh_bonus[0][pq][tid] = BA[pq];
            sh_bonus[1][pq][tid] = BB[pq];
        }
    };
    int pair = 0;  // 0 / 2: which two LDS images this iteration dumps into
    while (t < n_tiles) {
        f32x4 acc[2][NT];
        if (wid == 0 && lane < 32) {
            sh_tags[pair][lane] = R0.tag;
            sh_tags[pair + 1][lane] = R1.tag;
        }
        // the previous pair's bonus has arrived (requested before the loads whose tags were just stored): park it for this
        // iteration's ranking, then request this pair's, ahead of the refills below
        park_bonus();
#pragma unroll
        for (int pq = 0; pq < NT; ++pq) {
            BA[pq] = load_bonus(W0, pq);
            BB[pq] = load_bonus(W1, pq);
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
    park_bonus();
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
static hipError_t launch_boost_variant(const BoostArgs& a, int grid, hipStream_t stream) {
    constexpr size_t lds_bytes = (size_t)4 * kWaves * NT * 16 * kPitch * sizeof(float);  // 144 KiB at NT = 2
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&scan_boost_f32_kernel<CH, NT>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    hipLaunchKernelGGL((scan_boost_f32_kernel<CH, NT>), dim3(grid), dim3(kThreads), lds_bytes, stream, a);
    return hipGetLastError();
}

template <int NT>
static hipError_t launch_boost_ch(int ch, const BoostArgs& a, int grid, hipStream_t stream) {
    switch (ch) {
        case 1: return launch_boost_variant<1, NT>(a, grid, stream);
        case 2: return launch_boost_variant<2, NT>(a, grid, stream);
        case 3: return launch_boost_variant<3, NT>(a, grid, stream);
        case 4: return launch_boost_variant<4, NT>(a, grid, stream);
        case 5: return launch_boost_variant<5, NT>(a, grid, stream);
        case 6: return launch_boost_variant<6, NT>(a, grid, stream);
        case 7: return launch_boost_variant<7, NT>(a, grid, stream);
        case 8: return launch_boost_variant<8, NT>(a, grid, stream);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_scan_boost_f32(const BoostArgs& a, int grid, hipStream_t stream) {
    const ScanArgs& s = a.scan;
    if (s.row_stride % 128 != 0 || s.row_stride < 128 || s.row_stride > 1024) return hipErrorInvalidValue;   // narrow rows only
    if (s.nq < 1 || s.nq > 32 || s.k < 1 || s.k > 32 || s.n_rows < 1 || grid < 1) return hipErrorInvalidValue;
    if (!s.corpus || !s.q_padded || !s.part_scores || !s.part_ids || !a.bonus) return hipErrorInvalidValue;
    if ((s.q_after_score == nullptr) != (s.q_after_id == nullptr)) return hipErrorInvalidValue;
    if (s.q_filter_mask != nullptr && s.q_filter == nullptr) return hipErrorInvalidValue;
    if (s.q_filter != nullptr && s.row_tag == nullptr) return hipErrorInvalidValue;
    if (s.work_tile || s.work_base || s.sample_pass || s.sample_best || s.wgs_per_group || s.live_nq || s.allow || s.range_count ||
        s.group_table || s.count_table || s.id_base != 0)
        return hipErrorInvalidValue;
    // every in-range lane's offset lies inside the descriptor: (nq - 1) columns of bonus_q_stride, then bonus_rows values
    if (a.bonus_rows < 0 || a.bonus_q_stride < 0 || (a.bonus_q_stride > 0 && a.bonus_rows > a.bonus_q_stride)) return hipErrorInvalidValue;
    const int64_t need = ((int64_t)(a.bonus_q_stride > 0 ? s.nq - 1 : 0) * a.bonus_q_stride + a.bonus_rows) * 4;
    if (need > kBoostMaxBonusBytes || (int64_t)a.bonus_bytes != need) return hipErrorInvalidValue;
    if (a.transform != 0 && a.transform != 1) return hipErrorInvalidValue;
    const int ch = (int)(s.row_stride / 128);
    return s.nq <= 16 ? launch_boost_ch<1>(ch, a, grid, stream) : launch_boost_ch<2>(ch, a, grid, stream);
}

}  // namespace rass
