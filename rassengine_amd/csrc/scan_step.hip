// scan_step.hip — a run of consecutive query PAIRS of a fused fp32 batch in ONE launch (api_search.hip, scan_launch_batch).
//
// A 1 024-query step was 16 launches of scan_topk_f32_pair_kernel (scan_topk.hip), each a full pass over the slab for 64
// queries.  Every one of them paid, around an unchanged tile loop, for what being a launch of its own costs:
//   * tiles are dealt t = b + j * G, so with 31 250 tiles on 256 workgroups 18 of them run 123 iterations and 238 run 122 and
//     then wait one tile time for the launch to end — 1/123 of every pass;
//   * the prologue: 16 * CH query-fragment loads per lane, the first tile straight from HBM with nothing to overlap it, and a
//     20-bit radix selection of the wave's 8 sample floors, redone by every wave of every workgroup of every launch;
//   * the launch boundary itself.
// scan_topk_f32_step_kernel is that kernel's loop, with the same arithmetic — K split over the 8 waves, a tile multiplied as two
// 16-row blocks against 4 N-tiles of queries, one v_mfma_f32_16x16x4_f32 chain per (row, query) in k order from zero, the partials
// summed p0 + ... + p7 out of LDS, rank_load / rank_use wrapped around the same chunk slots — so every score is the pair
// kernel's bit for bit.  What changes is the sequence a workgroup walks: the `pairs * n_tiles` work items
// i = pair * n_tiles + tile, dealt i = b (mod G).  Within a pair a workgroup's tiles still ascend (the strict > of the
// insertion stays exact on ties), across pairs the remainder rotates by itself, and the only imbalance left is one item at the
// end of the whole launch.  The rolling refill follows the item sequence, so the rows of the next pair's first tile are in
// flight while the current pair finishes.  A workgroup switches pairs on its own (no grid barrier, no flag, no atomics): it
// ranks the last dumped tile, writes the pair's 8 lists per wave where the pair launch would have written them
// (part_* + pair * 2 * part_group_stride), resets its lists, reloads the query fragments from q_padded + pair * 2 *
// q_group_stride and refills the filters and the floors — ready-made, one per query (ScanArgs::step_floors, sample_rep.hip:
// step_floors_kernel) — between two barriers.
//
// The launcher asks for grid <= n_tiles (scan_grid gives that for every slab with a row): then a workgroup's next item is at
// most one pair on, the advance is branch-free, and every workgroup holds a tile of every pair, so every list of every pair is
// written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "scan_core.h"

namespace rass {

template <int CH>
__global__ __launch_bounds__(kThreads, 2) void scan_topk_f32_step_kernel(ScanArgs p) {
    constexpr int NT = 4, NQ = 64;
    extern __shared__ __attribute__((aligned(16))) float lds[];  // [2][kWaves][NQ][kPitch]

    const int lane = lane_id();
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = lane & 15, g = lane >> 4;
    const int G = gridDim.x, bid = blockIdx.x;
    const int n_tiles = (p.n_rows + kTileRows - 1) / kTileRows;
    const int pairs = p.nq_total / NQ;

    // Query fragments of a pair: lane (n = m, g) holds Qn[nt*16 + n][slice + 16j + 4g .. +3]; N-tiles 2, 3 are the pair's second group.
    f32x4 qf[NT][CH];
    auto load_queries = [&](int pair, int ln) {
        const int m = ln & 15, g = ln >> 4;
        const float* qbase = p.q_padded + (int64_t)pair * 2 * p.q_group_stride + (int64_t)m * p.row_stride + wid * 16 * CH + 4 * g;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const float* qn = qbase + (int64_t)(nt >> 1) * p.q_group_stride + (int64_t)(nt & 1) * 16 * p.row_stride;
#pragma unroll
            for (int j = 0; j < CH; ++j) qf[nt][j] = *reinterpret_cast<const f32x4*>(qn + 16 * j);
        }
    };
    load_queries(0, lane);
    const int voff_lane = wid * CH * 1024 + lane * 16;

    // Top-k state: pass pq handles query pq*16 + (lane>>5)*8 + wid of the pair for row lane&31.
    TopList L[NT];
    float tau[NT];
    auto reset_lists = [&]() {
#pragma unroll
        for (int pq = 0; pq < NT; ++pq) {
            L[pq].s = -INFINITY;
            L[pq].i = 0x7fffffff;
            tau[pq] = -INFINITY;
        }
    };
    reset_lists();
    __shared__ int sh_qfilt[NQ];
    __shared__ float sh_floor[NQ];
    __shared__ int sh_tags[2][32];
    // a pair's filters and floors (the floor of query q of the run: step_floors[q], what the pair kernel's prologue selects)
    auto fill_query_state = [&](int pair, int ln) {
        if (wid == 0) {
            const int q = pair * NQ + ln;
            sh_qfilt[ln] = p.q_filter != nullptr ? p.q_filter[q] : -1;
            sh_floor[ln] = p.step_floors != nullptr ? p.step_floors[q] : -INFINITY;
        }
    };
    fill_query_state(0, lane);
    __syncthreads();

    // item (pair, tile); past the last pair: no rows, a descriptor of zero records, nothing is fetched
    auto work = [&](int pair, int tile) {
        int rows = p.n_rows - tile * kTileRows;
        rows = rows > kTileRows ? kTileRows : rows;
        WorkItem w;
        w.tile = pair < pairs ? tile : 0;
        w.rows = pair < pairs ? rows : 0;
        w.mask = 0xffffffffu;
        return w;
    };

    const int mt_step = 16 * (int)p.row_stride * 4;
    HalfRegs<CH> R0, R1;  // the two 16-row blocks of the tile being multiplied; each register is refilled from the next item's tile
    int tag;
    int c_pair = 0, c_tile = bid;   // bid < G <= n_tiles
    WorkItem W0 = work(c_pair, c_tile);
    {
        const TileDesc d = make_tile_desc(p.corpus, p.row_stride, p.row_tag, W0);
        tag = load_tag(d);
        __builtin_amdgcn_sched_barrier(0);
        issue_half_loads<CH>(R0, d, voff_lane, 0);
        issue_half_loads<CH>(R1, d, voff_lane, mt_step);
    }
    __builtin_amdgcn_sched_barrier(0);

    auto dump_half = [&](const f32x4 (&acc)[NT], int buf, int blk) {
        float* P = lds + buf * (kWaves * NQ * kPitch);
        // lane (n=m, g) holds rows 4g..4g+3 of block blk for query nt*16+n
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
            *reinterpret_cast<f32x4*>(P + (wid * NQ + nt * 16 + m) * kPitch + blk * 16 + 4 * g) = acc[nt];
    };
    // The pair kernel's ranking, in its two steps: rank_load issues every LDS read of a part (the 8 K-partials, the row's tag,
    // the query's filter and floor), rank_use, one MFMA chunk later, sums the partials ((p0 + p1) + ...) + p7, filters with a
    // bitwise predicate and inserts.
    struct RankIn {
        float pz[kWaves];
        int tag, qfilt;
        float floor;
    };
    RankIn RI[NT];
    auto rank_load = [&](int buf, int pq) {
        const float* P = lds + buf * (kWaves * NQ * kPitch);
        const int r = lane & 31;
        const int q = pq * 16 + (lane >> 5) * 8 + wid;
        const float* src = P + q * kPitch + r;
#pragma unroll
        for (int wv = 0; wv < kWaves; ++wv) RI[pq].pz[wv] = src[wv * NQ * kPitch];
        RI[pq].tag = sh_tags[buf][r];
        RI[pq].qfilt = sh_qfilt[q];
        RI[pq].floor = sh_floor[q];
    };
    auto rank_use = [&](const WorkItem& w, int pq) {
        const int r = lane & 31;
        const int row = w.tile * kTileRows + r;
        const RankIn& in = RI[pq];
        float s = in.pz[0];
#pragma unroll
        for (int wv = 1; wv < kWaves; ++wv) s += in.pz[wv];
        // the sample floor: k rows of the corpus already score >= floor_q (ties are kept: the id order decides them in the merge)
        const bool ok = (r < w.rows) & (in.tag != -1) & ((in.qfilt < 0) | (in.qfilt == in.tag)) & (s >= in.floor);
        s = ok ? s : -INFINITY;
        insert_candidates(L[pq], tau[pq], s, row, p.k);
    };
    // A pair's per-workgroup sorted lists -> [gridDim.x][32][k] of each of its two groups
    auto write_lists = [&](int pair, int ln) {
        const int lpos = ln & 31;
#pragma unroll
        for (int pq = 0; pq < NT; ++pq) {
            const int ql = (pq & 1) * 16 + (ln >> 5) * 8 + wid;
            if (lpos < p.k) {
                const int64_t o = (int64_t)(pair * 2 + (pq >> 1)) * p.part_group_stride + ((int64_t)bid * 32 + ql) * p.k + lpos;
                const bool filled = L[pq].i != 0x7fffffff;
                p.part_scores[o] = filled ? L[pq].s : -INFINITY;
                p.part_ids[o] = filled ? (p.id_base + (int64_t)L[pq].i) : (int64_t)-1;
            }
        }
    };

    // Main loop: the pair kernel's iteration — multiply the item's tile, rank the previous item's out of the image it dumped,
    // parts at slots 1 / 5 / 9 / 13 (CH = 8), one barrier — over the item sequence.  Pw.rows = 0 after a switch: the first item
    // of a pair ranks nothing.
    auto slot_of = [](int part) { return (part * 2 * CH) / NT + (2 * CH > NT ? 1 : 0); };
    WorkItem Pw{0, 0, 0u};
    int cur = 0;            // which LDS image this iteration dumps into
    for (;;) {   // pairs >= 1 and bid < n_tiles (the launcher): the first item exists; the exit is in the switch below
        f32x4 acc[NT];
        if (wid == 0 && lane < 32) sh_tags[cur][lane] = tag;
        const WorkItem Wc = W0;
        int n_tile = c_tile + G, n_pair = c_pair;
        {
            const bool wrap = n_tile >= n_tiles;   // G <= n_tiles: at most once
            n_tile = wrap ? n_tile - n_tiles : n_tile;
            n_pair = wrap ? n_pair + 1 : n_pair;
        }
        const WorkItem Wn = work(n_pair, n_tile);
        const TileDesc dn = make_tile_desc(p.corpus, p.row_stride, p.row_tag, Wn);
        tag = load_tag(dn);
        auto load_prev = [&](int slot) {
#pragma unroll
            for (int part = 0; part < NT; ++part)
                if (slot_of(part) == slot) rank_load(cur ^ 1, part);
        };
        auto rank_prev = [&](int slot) {
#pragma unroll
            for (int part = 0; part < NT; ++part)
                if (slot_of(part) == slot) rank_use(Pw, part);
        };
        multiply_and_refill_half<CH, NT>(R0, qf, acc, dn, voff_lane, 0, [&](int j) { load_prev(j); },
                                         [&](int j) { rank_prev(j); });
        dump_half(acc, cur, 0);
        multiply_and_refill_half<CH, NT>(R1, qf, acc, dn, voff_lane, mt_step, [&](int j) { load_prev(CH + j); },
                                         [&](int j) { rank_prev(CH + j); });
        dump_half(acc, cur, 1);
        W0 = Wn;
        Pw = Wc;
        __syncthreads();
        cur ^= 1;
        c_tile = n_tile;
        // Workgroup-uniform and rare (once in n_tiles / G iterations): this was the workgroup's last tile of pair c_pair.  The
        // loop's exit sits inside, so that the back edge of every other iteration is the one branch behind the barrier, where
        // all 8 waves stand in lockstep and the matrix pipe waits for whatever the scalar unit does.
        if (__builtin_expect(n_pair != c_pair, 0)) {
#pragma unroll
            for (int pq = 0; pq < NT; ++pq) {
                rank_load(cur ^ 1, pq);
                rank_use(Pw, pq);
            }
            // Once per pair: the addresses below are recomputed from a lane id hipcc cannot see through.  Left visible, they are
            // loop invariants, hoisted and kept live across the tile loop, which has no register to spare at CH = 8 (6 spilled).
            int ln = lane;
            asm volatile("" : "+v"(ln));
            write_lists(c_pair, ln);
            if (n_pair >= pairs) break;
            reset_lists();
            Pw.rows = 0;
            c_pair = n_pair;
            load_queries(n_pair, ln);
            __syncthreads();   // every wave has ranked the pair's last tile: its filters and floors may go
            fill_query_state(n_pair, ln);
            __syncthreads();
            // The fragments are waited for HERE: left to their first use, their loads would be outstanding on one of the
            // edges into the loop top, and hipcc's s_waitcnt counts there — merged over every edge — would make every
            // iteration's first chunks wait for all of the tile's loads in flight instead of their own.
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int j = 0; j < CH; ++j) asm volatile("" : "+v"(qf[nt][j]));
        }
    }
}

template <int CH>
static hipError_t launch_step_variant(const ScanArgs& a, int grid, hipStream_t stream) {
    constexpr size_t lds_bytes = (size_t)2 * kWaves * 64 * kPitch * sizeof(float);  // 144 KiB
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&scan_topk_f32_step_kernel<CH>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    hipLaunchKernelGGL((scan_topk_f32_step_kernel<CH>), dim3(grid), dim3(kThreads), lds_bytes, stream, a);
    return hipGetLastError();
}

// a: the pair launch's arguments of the run's FIRST pair (q_padded, q_filter, part_* of its first group; nq = 64; the group
// strides), nq_total = 64 * pairs, step_floors = the floors of the run's queries or nullptr (none: -inf), sample_best unused.
hipError_t launch_scan_topk_f32_step(const ScanArgs& a, int grid, hipStream_t stream) {
    if (!scan_pair_supported_stride(a.row_stride)) return hipErrorInvalidValue;
    const int pairs = a.nq_total / 64;
    if (a.nq != 64 || a.nq_total != 64 * pairs || pairs < 1 || pairs > kStepMaxPairs || a.q_group_stride <= 0 ||
        a.part_group_stride <= 0)
        return hipErrorInvalidValue;
    if (grid < 1 || grid > (a.n_rows + kTileRows - 1) / kTileRows) return hipErrorInvalidValue;
    if (a.q_filter_mask || a.q_after_score || a.q_after_id || a.work_tile || a.work_base || a.sample_pass || a.live_nq ||
        a.wgs_per_group || a.sample_best)
        return hipErrorInvalidValue;
    switch ((int)(a.row_stride / 128)) {
        case 1: return launch_step_variant<1>(a, grid, stream);
        case 2: return launch_step_variant<2>(a, grid, stream);
        case 3: return launch_step_variant<3>(a, grid, stream);
        case 4: return launch_step_variant<4>(a, grid, stream);
        case 5: return launch_step_variant<5>(a, grid, stream);
        case 6: return launch_step_variant<6>(a, grid, stream);
        case 7: return launch_step_variant<7>(a, grid, stream);
        case 8: return launch_step_variant<8>(a, grid, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace rass
