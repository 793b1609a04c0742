// scan_topk.hip — K1+K2 of SURVEY §8a: fused flat cosine scan + top-k for gfx950.
//
// Replaces the arithmetic behind OpenSearchIndexer.semantic_search's knn query
// (reference app/main.py:1527-1560; HNSW walk in the k-NN plugin) with an exact
// scan: S[q][row] = <Qn[q], Xn[row]> over a row-major fp32 corpus resident in HBM,
// top-k per query under the total order (score desc, id asc).
//
// Shape of the kernel (one 512-thread workgroup per CU, persistent over row tiles):
//   * HBM layout ("tile16", kernels.h): the corpus is stored in 16-row blocks; inside a block
//     the 16 rows x 16 columns (64 B each) of chunk j are ONE contiguous 1 KiB in MFMA lane
//     order, lane (m = lane&15, g = lane>>4) <-> X[16b+m][16j + 4g .. +3].  So every wave-level
//     load is a fully coalesced 1 KiB burst that lands directly in A-operand layout (measured:
//     6.6 TB/s for this pattern vs 5.6 TB/s for 16 rows x 64 B fragment-shaped loads from a
//     plain row-major slab; scripts/microbench/stream_patterns.hip)
//   * a tile is 32 corpus rows (two blocks); the 8 waves split the K (=dim) axis, wave w owns
//     chunks [w*CH, (w+1)*CH) of every block (dim_padded = 128*CH)
//   * corpus bytes go HBM -> VGPR directly (read-once stream, GEMV-shaped: no LDS
//     round trip), 16 B per lane, as the A operand of v_mfma_f32_16x16x4_f32
//   * the query fragments (B operand) stay in registers for the whole launch
//   * loads are buffer loads through a per-tile descriptor, so rows past n_rows and
//     the run-ahead prefetch of a tile past the end cost no HBM traffic (range check)
//   * two register tile buffers per wave; each 16 B register is re-loaded for the tile two
//     steps ahead right after the MFMAs that consumed it, so ~32 KiB per wave (256 KiB per
//     CU) stay in flight continuously; ONE VGPR carries the lane's load offset, the M-tile /
//     chunk part goes into the instruction's SGPR and immediate offset fields
//   * per tile, each wave dumps its 32x(16*NT) partial scores to LDS; two tiles share one barrier
//     (four LDS images).  The RANKING of a tile pair — wave w sums the 8 K-partials of "its" queries
//     in a fixed order, filters by threshold (ballot) and inserts into the half-wave sorted lists —
//     runs one iteration later, cut into 2*NT parts placed BETWEEN the MFMA chunks of the next pair,
//     so its LDS reads and VALU work issue while the matrix pipe executes (round 1 ranked in a phase
//     of its own behind the barrier: the pipe idled while all 8 waves ranked, 72 us of 690 at B = 32;
//     profiles/r02_scan_phase_experiments.txt).  Row tags and per-query filters live in LDS
//   * the insertion itself is register / scalar only: DPP wave_shr for the shift, readlane for the
//     broadcasts, bitwise predicates + selects instead of exec-mask branches (scan_core.h)
//   * at the end each workgroup writes a sorted top-k list per query; merge_topk.hip
//     reduces [n_workgroups][nq][k] -> [nq][k]
//   * EXT variant (template flag, same main loop): masked tag filters and the continuation bound of
//     a multi-pass top-k (k > 32), parameters in LDS
//
// Numerics: v_mfma_f32_16x16x4_f32 is an exact f32 fmaf chain in k order, so a score is
// a fixed sequence of fmaf's per K-slice followed by 7 f32 adds: independent of the grid,
// of the shard split and of the query batch (oracle/rass_oracle.c restates that order
// on the CPU and the GPU tests require bit-equality with it).
//
// Algorithmic bytes per launch (roofline.achieved in bench.py): n_rows * row_stride * 4.
// The corpus must be allocated in whole 16-row blocks (rows past n_rows are masked).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "scan_core.h"

namespace rass {

#ifdef RASS_SCAN_DIAG  // diagnostic builds only (scripts/probe_scan_diag.py): launch-wide event counters
// [0] ranking calls, [1] calls with >= 1 candidate, [2] candidates, [4] candidates the sample floor rejected
__device__ unsigned long long g_scan_diag[8];
#endif

#ifdef RASS_SCAN_CLOCKS  // scripts/microbench/scan_tail.hip only: per-workgroup start / end wall clocks
__device__ unsigned long long g_scan_clocks[2 * 1024];
__device__ unsigned long long g_scan_core[2];
#endif

// The ascending sequence of work-item indices one workgroup handles.  Plain: b, b+G, b+2G, ...
// With XCD skew s: the items are cut into super-rounds of s*G + G/2; in each, every workgroup
// takes s items round-robin (j*G + b) and the even workgroups one more (s*G + b/2).
struct ItemSeq {
    int base, j, lim, skew, G, b, period;
    __device__ __forceinline__ ItemSeq(int b_, int G_, int skew_) : base(0), j(0), skew(skew_), G(G_), b(b_) {
        lim = skew == 0 ? 1 : ((b & 1) ? skew : skew + 1);
        period = skew == 0 ? G : skew * G + (G >> 1);
    }
    __device__ __forceinline__ int next() {
        const int r = (skew == 0 || j < skew) ? base + j * G + b : base + skew * G + (b >> 1);
        if (++j == lim) {
            j = 0;
            base += period;
        }
        return r;
    }
};

template <int MODE>
__device__ __forceinline__ WorkItem get_work(const ScanArgs& p, int i, int n_items) {
    WorkItem w;
    if (!mode_is_flat(MODE)) {
        const bool ok = i < n_items;
        w.tile = ok ? p.work_tile[i] : 0;
        w.rows = ok ? p.work_rows[i] : 0;
        w.mask = ok ? p.work_mask[i] : 0u;
    } else {
        int rows = p.n_rows - i * kTileRows;
        rows = rows < 0 ? 0 : (rows > kTileRows ? kTileRows : rows);
        w.tile = i < n_items ? i : 0;
        w.rows = i < n_items ? rows : 0;
        w.mask = 0xffffffffu;
    }
    return w;
}

// The slab / tag array a work item streams: the launch's one slab, or (MULTI) the item's own.  `i` past the end
// reads item 0's pointers (rows = 0 there, so the descriptor has zero records and nothing is fetched).
template <int MODE>
__device__ __forceinline__ const float* slab_of(const ScanArgs& p, int i, int n_items) {
    return MODE == kMulti ? p.work_base[i < n_items ? i : 0] : p.corpus;
}
template <int MODE>
__device__ __forceinline__ const int32_t* tags_of(const ScanArgs& p, int i, int n_items) {
    return MODE == kMulti ? p.work_tags[i < n_items ? i : 0] : p.row_tag;
}

template <int CH, int NT, int MODE, bool EXT>
__global__ __launch_bounds__(kThreads, 2) void scan_topk_f32_kernel(ScanArgs p) {
    constexpr bool IVF = !mode_is_flat(MODE);  // a work list with per-item query masks
    constexpr int NQ = NT * 16;
    extern __shared__ __attribute__((aligned(16))) float lds[];  // [4][kWaves][NQ][kPitch]

    const int lane = lane_id();
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = lane & 15, g = lane >> 4;
    if (p.live_nq != nullptr && __builtin_amdgcn_readfirstlane(*p.live_nq) == 0) return;
    // number of work items: tiles of the slab (flat) or entries of the probe plan (IVF; written
    // by plan_probe_kernel earlier on this stream)
    int G = gridDim.x;
    int bid = blockIdx.x;   // this workgroup's position among the G that share its queries
    if (MODE == kFlatGroups || MODE == kIvfGroups || MODE == kFlatSampleGroups) {
        const int grp = bid / p.wgs_per_group;
        bid -= grp * p.wgs_per_group;
        G = p.wgs_per_group;
        p.q_padded += (int64_t)grp * p.q_group_stride;
        p.part_scores += (int64_t)grp * p.part_group_stride;
        if (MODE != kFlatSampleGroups) p.part_ids += (int64_t)grp * p.part_group_stride;
        if (p.q_filter != nullptr) p.q_filter += grp * 32;
        if (MODE == kFlatSampleGroups) p.nq = min(32, p.nq_total - 32 * grp);
        if (MODE == kIvfGroups) {
            p.work_tile += (int64_t)grp * p.work_group_stride;
            p.work_rows += (int64_t)grp * p.work_group_stride;
            p.work_mask += (int64_t)grp * p.work_group_stride;
            p.n_work += grp;
            p.nq = min(32, p.nq_total - 32 * grp);
        }
    }
    const int n_tiles = IVF ? __builtin_amdgcn_readfirstlane(*p.n_work) : (p.n_rows + kTileRows - 1) / kTileRows;
#ifdef RASS_SCAN_CLOCKS
    if (threadIdx.x == 0) g_scan_clocks[2 * blockIdx.x] = wall_clock64();
    if (threadIdx.x == 0 && blockIdx.x == 0) g_scan_core[0] = clock64();
#endif

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
    // Byte offset of this lane inside a tile: block 0, this wave's chunk 0, 16 B per lane.
    const int voff_lane = wid * CH * 1024 + lane * 16;

    // Top-k state: pass pq handles query pq*16 + (lane>>5)*8 + wid for row lane&31.
    TopList L[NT];
    float tau[NT];
#pragma unroll
    for (int pq = 0; pq < NT; ++pq) {
        L[pq].s = -INFINITY;
        L[pq].i = 0x7fffffff;
        tau[pq] = -INFINITY;
    }
    // Per-query filter parameters and the dumped tiles' row tags live in LDS (1.5 KiB next to the 144 KiB of
    // partial images), not in registers: they are read in the ranking step only, and the main loop has no VGPRs
    // to spare at CH = 8, NT = 2 (the ranking runs between the MFMA chunks, so its operands are live there).
    __shared__ int sh_qfilt[32];
    __shared__ float sh_floor[32];  // the launch's per-query score floors (ScanArgs::sample_best), -inf without
    __shared__ int sh_tags[4][32];
    __shared__ int sh_qmask[32];
    __shared__ float sh_after_s[32];
    __shared__ int64_t sh_after_i[32];
    __shared__ float sh_thr[32];    // kRange, kGroupCount: the per-query score thresholds (NaN past nq: nothing matches)
    __shared__ int sh_keys[4][32];  // kGroupMaxKeys, kGroupCountKeys: the dumped tiles' group keys, next to their tags
    constexpr bool KEYS = mode_has_keys(MODE);
    if (threadIdx.x < 32) {
        const int q = threadIdx.x;
        const bool live = q < p.nq;
        sh_qfilt[q] = (p.q_filter != nullptr && live) ? p.q_filter[q] : -1;
        sh_floor[q] = -INFINITY;
        if (MODE == kRange || MODE == kGroupCount || MODE == kGroupCountKeys) sh_thr[q] = live ? p.range_thr[q] : __builtin_nanf("");
        if (EXT) {
            sh_qmask[q] = (p.q_filter_mask != nullptr && live) ? p.q_filter_mask[q] : -1;
            sh_after_s[q] = (p.q_after_score != nullptr && live) ? p.q_after_score[q] : INFINITY;
            sh_after_i[q] = (p.q_after_id != nullptr && live) ? p.q_after_id[q] : (int64_t)-1;
        }
    }
    __syncthreads();

    // The sample pass's per-workgroup best scores of this wave's 2 x NT queries, as order-preserving keys (0 = none):
    // loaded BEFORE the first tiles so that the selection below runs while those are in flight.
    unsigned best_key[NT][2][kMaxSampleGroups / 64];
    if (MODE == kFlat && p.sample_best != nullptr) {
#pragma unroll
        for (int pq = 0; pq < NT; ++pq)
#pragma unroll
            for (int half = 0; half < 2; ++half)
#pragma unroll
                for (int j = 0; j < kMaxSampleGroups / 64; ++j) {
                    const int grp = lane + 64 * j;
                    const float v = grp < p.sample_groups ? p.sample_best[(pq * 16 + half * 8 + wid) * kMaxSampleGroups + grp] : -INFINITY;
                    best_key[pq][half][j] = v == -INFINITY ? 0u : score_key(v);
                }
    }

    const int mt_step = 16 * (int)p.row_stride * 4;
    TileRegs<CH> R0, R1;
    ItemSeq seq(bid, G, (G & 1) ? 0 : p.xcd_skew);
    int t = seq.next();  // the item R0 holds; R1 holds the one after it
    const int t1 = seq.next();
    WorkItem W0 = get_work<MODE>(p, t, n_tiles), W1 = get_work<MODE>(p, t1, n_tiles);
    // KEYS: the two tiles' group keys, one register each, requested AHEAD of the tiles' own loads here and in the main loop: the
    // wait that parks a tile's tags in LDS has then seen the older key load come back too (vmcnt counts in order)
    int K0 = 0, K1 = 0;
    if (KEYS) {
        K0 = load_tile_keys(p.group_keys, p.group_key_rows, W0);
        K1 = load_tile_keys(p.group_keys, p.group_key_rows, W1);
    }
    issue_tile_loads<CH>(R0, make_tile_desc(slab_of<MODE>(p, t, n_tiles), p.row_stride, tags_of<MODE>(p, t, n_tiles), W0),
                         voff_lane, mt_step);
    issue_tile_loads<CH>(R1, make_tile_desc(slab_of<MODE>(p, t1, n_tiles), p.row_stride, tags_of<MODE>(p, t1, n_tiles), W1),
                         voff_lane, mt_step);
    __builtin_amdgcn_sched_barrier(0);

    // The sample floor of each of this wave's queries: the k-th largest of the sample pass's per-workgroup bests
    // (those workgroups scanned disjoint rows, so k rows of the slab reach it under the query's filters, and so
    // does the final k-th best; fewer than k finite entries: no floor).  Radix selection over the keys' top
    // kFloorBits bits (scan_core.h) by ballot counts.
    if (MODE == kFlat && p.sample_best != nullptr) {
        unsigned T[NT][2] = {};
        // bit by bit, the wave's 2 x NT selections side by side (each is a chain of dependent scalar steps)
#pragma unroll 1
        for (int b = 31; b >= 32 - kFloorBits; --b) {
#pragma unroll
            for (int pq = 0; pq < NT; ++pq)
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const unsigned cand = T[pq][half] | (1u << b);
                    int c = 0;
#pragma unroll
                    for (int j = 0; j < kMaxSampleGroups / 64; ++j) c += __popcll(__ballot(best_key[pq][half][j] >= cand));
                    T[pq][half] = c >= p.k ? cand : T[pq][half];
                }
        }
#pragma unroll
        for (int pq = 0; pq < NT; ++pq)
#pragma unroll
            for (int half = 0; half < 2; ++half)
                if (lane == 0) sh_floor[pq * 16 + half * 8 + wid] = T[pq][half] ? key_score(T[pq][half]) : -INFINITY;
    }

    // A tile's 8 K-partials meet in LDS.  Two tiles share ONE barrier: both are dumped (four LDS
    // images: two per loop iteration, alternating between iterations so a fast wave's next dump never
    // lands on an image a slow wave is still reading — it would have to pass the next barrier first),
    // then ranked in ascending row order.
    auto dump_tile = [&](const f32x4 (&acc)[2][NT], int buf) {
        float* P = lds + buf * (kWaves * NQ * kPitch);
        // lane (n=m, g) holds rows 4g..4g+3 of M-tile mt for query nt*16+n
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                *reinterpret_cast<f32x4*>(P + (wid * NQ + nt * 16 + m) * kPitch + mt * 16 + 4 * g) = acc[mt][nt];
    };
#ifdef RASS_SCAN_DIAG
    unsigned d_calls = 0, d_any = 0, d_cand = 0, d_rej = 0;
#endif
    // Rank one (tile, query group pq) of a dumped tile: sum the 8 K-partials in fixed order, filter, insert.
    auto rank_part = [&](const WorkItem& w, int buf, int pq) {
        const float* P = lds + buf * (kWaves * NQ * kPitch);
        const int r = lane & 31;
        const int row = w.tile * kTileRows + r;
        const int tag = sh_tags[buf][r];
        const bool row_ok = (r < w.rows) && (tag != -1);
        const int q = pq * 16 + (lane >> 5) * 8 + wid;
        const int qf1 = sh_qfilt[q];
        const float* src = P + q * kPitch + r;
        float s = src[0];
#pragma unroll
        for (int wv = 1; wv < kWaves; ++wv) s += src[wv * NQ * kPitch];
        bool ok;
        if (EXT) {
            ok = row_ok && (qf1 < 0 || qf1 == (tag & sh_qmask[q]));
            // continuation: strictly after (after_s, after_i) in (score desc, id asc)
            const float as = sh_after_s[q];
            ok = ok && (s < as || (s == as && (p.id_base + (int64_t)row) > sh_after_i[q]));
        } else {
            ok = row_ok && (qf1 < 0 || qf1 == tag);
        }
        if (IVF) ok = ok && ((w.mask >> q) & 1u);
        if (MODE == kAllow) {
            // the row's bit in its query's word of the tile.  The wave's two queries of this part (one per half) and the tile
            // are wave-uniform, so the two words come by scalar loads: no vector register, no LDS, and no wait on the corpus
            // loads in flight.  Queries past nq (zero rows, never written) read the last live query's word: in bounds.
            const int qa = min(pq * 16 + wid, p.nq - 1), qb = min(pq * 16 + 8 + wid, p.nq - 1);
            const unsigned wa = p.allow[(int64_t)qa * p.allow_q_stride + w.tile];
            const unsigned wb = p.allow[(int64_t)qb * p.allow_q_stride + w.tile];
            ok = ok && ((((lane & 32) ? wb : wa) >> r) & 1u);
        }
        if (MODE == kRange) {   // no ranking: count and emit the rows at or above the query's threshold
            emit_range(ok && s >= sh_thr[q], s, row, p.range_count + q * kRangeCountStride, p.range_hits + (int64_t)q * p.range_cap,
                       p.range_cap);
            return;
        }
        if (MODE == kGroupMax) {   // no ranking either: the row's key goes into its (query, group) slot
            emit_group_max(ok && q < p.nq, s, row, tag, p.group_mask, p.group_shift, p.group_n,
                           p.group_table + (int64_t)q * p.group_n, p.group_status);
            return;
        }
        if (MODE == kGroupCount) {   // kRange's hits, counted per (query, group) slot; the slot's best row as kGroupMax keeps it
            emit_group_count(ok && s >= sh_thr[q], s, row, tag, q, p.group_mask, p.group_shift, p.group_n, p.group_table, p.count_table,
                             p.group_status);
            return;
        }
        if (KEYS) {   // the two emissions above with the row's group from its key column, within the bitmap where there is one
            const int key = sh_keys[buf][r];
            ok = ok && key >= 0 && row < p.group_key_rows;   // no group: neither a match nor a hit, whatever the key's size
            if (p.allow != nullptr) {   // kAllow's test (a kernel argument: a scalar branch, not an exec mask)
                // The wave's two words of the tile.  This kernel also writes global memory (the emitters' atomics), so hipcc
                // no longer proves a plain load of the bitmap unclobbered and would fetch it with a vector load and a
                // vmcnt(0) wait right here, between the MFMA chunks, draining the corpus loads in flight.  Read through
                // the constant address space the two wave-uniform addresses are scalar loads whatever else the kernel does.
                typedef const __attribute__((address_space(4))) unsigned* const_words;
                const const_words allow = (const_words)reinterpret_cast<uintptr_t>(p.allow);
                const int qa = min(pq * 16 + wid, p.nq - 1), qb = min(pq * 16 + 8 + wid, p.nq - 1);
                const unsigned wa = allow[(int64_t)qa * p.allow_q_stride + w.tile];
                const unsigned wb = allow[(int64_t)qb * p.allow_q_stride + w.tile];
                ok = ok && ((((lane & 32) ? wb : wa) >> r) & 1u);
            }
            // the whole key is the group: mask 0x7fffffff, shift 0
            if (MODE == kGroupMaxKeys)
                emit_group_max(ok && q < p.nq, s, row, key, 0x7fffffff, 0, p.group_n, p.group_table + (int64_t)q * p.group_n,
                               p.group_status);
            else
                emit_group_count(ok && s >= sh_thr[q], s, row, key, q, 0x7fffffff, 0, p.group_n, p.group_table, p.count_table,
                                 p.group_status);
            return;
        }
        // the sample floor: k rows of the corpus already score >= floor_q, so a row below it cannot be in the
        // query's top-k (ties are kept: the id order decides them in the merge)
        const float floor_q = MODE == kFlat ? sh_floor[q] : -INFINITY;
#ifdef RASS_SCAN_DIAG
        d_rej += __popcll(__ballot(ok && s > tau[pq] && s < floor_q));
#endif
        if (MODE == kFlat) ok = ok && (s >= floor_q);
        s = ok ? s : -INFINITY;
#ifdef RASS_SCAN_DIAG
        {
            const int c = __popcll(__ballot(s > tau[pq]));
            d_calls += 1; d_any += c != 0; d_cand += c;
        }
#endif
        if (mode_is_sample(MODE))
            L[pq].s = fmaxf(L[pq].s, s);  // the sample pass keeps each row slot's best score, nothing else
        else
            insert_candidates(L[pq], tau[pq], s, row, p.k);
    };

    // Main loop.  Iteration i multiplies the tile pair (A_i, B_i) and, between the MFMA chunks, ranks the pair
    // of iteration i-1 out of the LDS images that iteration dumped (2 x NT parts spread over the 2 x CH chunk
    // slots; rows are still ranked in ascending order, which the strict `>` tie rule needs).  One barrier per
    // iteration: it orders this iteration's dumps before the next iteration's reads, and the next iteration's
    // dumps (into the images read now) behind this iteration's reads.
    constexpr int kParts = 2 * NT;
    // (max: at CH = 1, NT = 2 there are 2 slots for 4 parts and part 0 would land in slot -1 — never ranked, its rows lost)
    auto slot_of = [](int part) { return max(((part + 1) * 2 * CH) / kParts - 1, 0); };
    WorkItem Pa{0, 0, 0u}, Pb{0, 0, 0u};  // the previous pair (rows = 0: nothing ranks in the first iteration)
    int pair = 0;  // 0 / 2: which two LDS images this iteration dumps into
    while (t < n_tiles) {
        f32x4 acc[2][NT];
        // the pair's row tags go to LDS now (every wave loaded the same 32 per tile): the refill below reuses
        // R.tag for the tile two steps ahead, and the ranking reads them an iteration later
        if (wid == 0 && lane < 32) {
            sh_tags[pair][lane] = R0.tag;
            sh_tags[pair + 1][lane] = R1.tag;
            if (KEYS) {
                sh_keys[pair][lane] = K0;
                sh_keys[pair + 1][lane] = K1;
            }
        }
        const WorkItem Wa = W0;
        t = seq.next();
        WorkItem Wn = get_work<MODE>(p, t, n_tiles);
        if (KEYS) K0 = load_tile_keys(p.group_keys, p.group_key_rows, Wn);
        auto rank_prev = [&](int slot) {
#pragma unroll
            for (int part = 0; part < kParts; ++part)
                if (slot_of(part) == slot) {
                    if (part < NT)
                        rank_part(Pa, pair ^ 2, part);
                    else
                        rank_part(Pb, (pair ^ 2) + 1, part - NT);
                }
        };
        multiply_and_refill<CH, NT>(R0, qf, acc,
                                    make_tile_desc(slab_of<MODE>(p, t, n_tiles), p.row_stride, tags_of<MODE>(p, t, n_tiles), Wn),
                                    voff_lane, mt_step, [&](int j) { rank_prev(j); });
        dump_tile(acc, pair);
        W0 = Wn;
        const WorkItem Wb = W1;
        const int tn = seq.next();
        Wn = get_work<MODE>(p, tn, n_tiles);
        if (KEYS) K1 = load_tile_keys(p.group_keys, p.group_key_rows, Wn);
        multiply_and_refill<CH, NT>(R1, qf, acc,
                                    make_tile_desc(slab_of<MODE>(p, tn, n_tiles), p.row_stride, tags_of<MODE>(p, tn, n_tiles), Wn),
                                    voff_lane, mt_step, [&](int j) { rank_prev(CH + j); });
        dump_tile(acc, pair + 1);
        W1 = Wn;
        Pa = Wa;
        Pb = Wb;
        __syncthreads();
        pair ^= 2;
    }
    // the last pair
#pragma unroll
    for (int pq = 0; pq < NT; ++pq) rank_part(Pa, pair ^ 2, pq);
#pragma unroll
    for (int pq = 0; pq < NT; ++pq) rank_part(Pb, (pair ^ 2) + 1, pq);

#ifdef RASS_SCAN_DIAG
    if (lane == 0) {
        atomicAdd(&g_scan_diag[0], (unsigned long long)d_calls);
        atomicAdd(&g_scan_diag[1], (unsigned long long)d_any);
        atomicAdd(&g_scan_diag[2], (unsigned long long)d_cand);
        atomicAdd(&g_scan_diag[4], (unsigned long long)d_rej);
    }
#endif
#ifdef RASS_SCAN_CLOCKS
    if (threadIdx.x == 0) g_scan_clocks[2 * blockIdx.x + 1] = wall_clock64();
    if (threadIdx.x == 0 && blockIdx.x == 0) g_scan_core[1] = clock64();
#endif
    if (MODE == kRange || MODE == kGroupMax || MODE == kGroupCount || KEYS) return;   // everything was emitted on the way
    if (mode_is_sample(MODE)) {
        // The sample pass: this workgroup's best score per query -> part_scores[32][kMaxSampleGroups] (-inf: no row of the
        // sample passed the query's filters); the big scan's waves take the k-th largest over the workgroups.
#pragma unroll
        for (int pq = 0; pq < NT; ++pq) {
            float v = L[pq].s;
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 32));
            const int q = pq * 16 + (lane >> 5) * 8 + wid;
            if ((lane & 31) == 0) p.part_scores[q * kMaxSampleGroups + bid] = q < p.nq ? v : -INFINITY;
        }
        return;
    }
    // Per-workgroup sorted lists -> [gridDim.x][nq][k]
    const int lpos = lane & 31;
#pragma unroll
    for (int pq = 0; pq < NT; ++pq) {
        const int q = pq * 16 + (lane >> 5) * 8 + wid;
        if (q < p.nq && lpos < p.k) {
            const int64_t o = ((int64_t)bid * p.nq + q) * p.k + lpos;
            const bool filled = L[pq].i != 0x7fffffff;
            p.part_scores[o] = filled ? L[pq].s : -INFINITY;
            p.part_ids[o] = filled ? (p.id_base + (int64_t)L[pq].i) : (int64_t)-1;
        }
    }
}

// ------------------------------------------------------------------------------------------
// 64 queries per corpus pass: TWO consecutive full launch groups of a batch call in one launch (api_search.hip,
// scan_launch_batch).  At 32 queries per pass the kernel above sits in the corner of the HBM rate and the fp32 MFMA
// rate; a step of 1 024 queries streams the corpus 32 times.  This sibling streams it 16 times: the same 512 threads,
// the same K split over the 8 waves and the same v_mfma_f32_16x16x4_f32 chain per (row, query) in k order from zero,
// the same p0 + ... + p7 sum of the partials — so every score is the kernel above's, bit for bit — but a tile is
// multiplied as two 16-row blocks against 4 N-tiles of queries (HalfRegs / multiply_and_refill_half, scan_core.h)
// instead of two blocks together against 2.  Registers at CH = 8: 128 for the query fragments (64 above), 2 x 32 for
// the two blocks of ONE tile in flight (2 x 64 above: half the bytes per MFMA want half the bytes in flight), 16
// accumulators.  The LDS image of a tile is [kWaves][64][kPitch]: block 0's rows in columns 0..15, block 1's in
// 16..31, so the dump and the ranking address it exactly as above (same pitch, same bank pattern), and a half-wave
// still ranks the 32 rows of a tile for one query in ascending row order.  One tile and one barrier per iteration
// (256 MFMAs per wave, as above), two images; the previous tile's ranking is cut into 4 parts (one per N-tile: a wave
// owns queries pq * 16 + {0, 8} + wid, 8 of them), each wrapped AROUND one MFMA chunk: its LDS reads are issued ahead of the
// chunk's 16 MFMAs and consumed behind them (rank_load / rank_use below).  The 8 waves run in lockstep behind the per-tile
// barrier, so whatever the ranking waits for behind a chunk, the matrix pipe waits for too: no LDS round trip is left there.
// 1 087 -> 1 069 us per pass at CH = 8, 27 % of what the ranking cost (DESIGN.md s3,
// profiles/scan_pair_rank_prefetch_experiment.txt).
// Queries 0..31 are group g's (q_padded, q_filter, sample_best, part_*), 32..63 group g + 1's: q_padded +
// q_group_stride, q_filter + 32, sample_best + 32 * kMaxSampleGroups, part_* + part_group_stride — where the two
// launches it replaces read and write.  Flat scans without EXT only.
template <int CH>
__global__ __launch_bounds__(kThreads, 2) void scan_topk_f32_pair_kernel(ScanArgs p) {
    constexpr int NT = 4, NQ = 64;
    extern __shared__ __attribute__((aligned(16))) float lds[];  // [2][kWaves][NQ][kPitch]

    const int lane = lane_id();
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = lane & 15, g = lane >> 4;
    const int G = gridDim.x, bid = blockIdx.x;
    const int n_tiles = (p.n_rows + kTileRows - 1) / kTileRows;

    // Query fragments: lane (n = m, g) holds Qn[nt*16 + n][slice + 16j + 4g .. +3]; N-tiles 2, 3 are the second group's.
    f32x4 qf[NT][CH];
    {
        const float* qbase = p.q_padded + (int64_t)m * p.row_stride + wid * 16 * CH + 4 * g;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const float* qn = qbase + (int64_t)(nt >> 1) * p.q_group_stride + (int64_t)(nt & 1) * 16 * p.row_stride;
#pragma unroll
            for (int j = 0; j < CH; ++j) qf[nt][j] = *reinterpret_cast<const f32x4*>(qn + 16 * j);
        }
    }
    const int voff_lane = wid * CH * 1024 + lane * 16;

    // Top-k state: pass pq handles query pq*16 + (lane>>5)*8 + wid for row lane&31.
    TopList L[NT];
    float tau[NT];
#pragma unroll
    for (int pq = 0; pq < NT; ++pq) {
        L[pq].s = -INFINITY;
        L[pq].i = 0x7fffffff;
        tau[pq] = -INFINITY;
    }
    __shared__ int sh_qfilt[NQ];
    __shared__ float sh_floor[NQ];
    __shared__ int sh_tags[2][32];
    if (threadIdx.x < NQ) {
        sh_qfilt[threadIdx.x] = p.q_filter != nullptr ? p.q_filter[threadIdx.x] : -1;
        sh_floor[threadIdx.x] = -INFINITY;
    }
    __syncthreads();

    const int mt_step = 16 * (int)p.row_stride * 4;
    HalfRegs<CH> R0, R1;  // the two 16-row blocks of the tile being multiplied; each register is refilled from the next tile
    int tag;
    ItemSeq seq(bid, G, (G & 1) ? 0 : p.xcd_skew);
    int t = seq.next();
    WorkItem W0 = get_work<kFlat>(p, t, n_tiles);
    {
        const TileDesc d = make_tile_desc(p.corpus, p.row_stride, p.row_tag, W0);
        tag = load_tag(d);
        __builtin_amdgcn_sched_barrier(0);
        issue_half_loads<CH>(R0, d, voff_lane, 0);
        issue_half_loads<CH>(R1, d, voff_lane, mt_step);
    }
    __builtin_amdgcn_sched_barrier(0);

    // The sample floors of this wave's 8 queries, as in the kernel above (same keys, same selection, same floors), one
    // launch group after the other: the keys of 4 queries take 16 registers next to the 128 of the query fragments.
    if (p.sample_best != nullptr) {
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
            unsigned best_key[2][2][kMaxSampleGroups / 64];
#pragma unroll
            for (int pq = 0; pq < 2; ++pq)
#pragma unroll
                for (int half = 0; half < 2; ++half)
#pragma unroll
                    for (int j = 0; j < kMaxSampleGroups / 64; ++j) {
                        const int grp = lane + 64 * j;
                        const int q = h * 32 + pq * 16 + half * 8 + wid;
                        const float v = grp < p.sample_groups ? p.sample_best[q * kMaxSampleGroups + grp] : -INFINITY;
                        best_key[pq][half][j] = v == -INFINITY ? 0u : score_key(v);
                    }
            unsigned T[2][2] = {};
#pragma unroll 1
            for (int b = 31; b >= 32 - kFloorBits; --b) {
#pragma unroll
                for (int pq = 0; pq < 2; ++pq)
#pragma unroll
                    for (int half = 0; half < 2; ++half) {
                        const unsigned cand = T[pq][half] | (1u << b);
                        int c = 0;
#pragma unroll
                        for (int j = 0; j < kMaxSampleGroups / 64; ++j) c += __popcll(__ballot(best_key[pq][half][j] >= cand));
                        T[pq][half] = c >= p.k ? cand : T[pq][half];
                    }
            }
#pragma unroll
            for (int pq = 0; pq < 2; ++pq)
#pragma unroll
                for (int half = 0; half < 2; ++half)
                    if (lane == 0) sh_floor[h * 32 + pq * 16 + half * 8 + wid] = T[pq][half] ? key_score(T[pq][half]) : -INFINITY;
        }
    }

    auto dump_half = [&](const f32x4 (&acc)[NT], int buf, int blk) {
        float* P = lds + buf * (kWaves * NQ * kPitch);
        // lane (n=m, g) holds rows 4g..4g+3 of block blk for query nt*16+n
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
            *reinterpret_cast<f32x4*>(P + (wid * NQ + nt * 16 + m) * kPitch + blk * 16 + 4 * g) = acc[nt];
    };
    // Rank one (tile, N-tile pq) of a dumped tile, in two steps.  rank_load issues EVERY LDS read of the part, unconditionally
    // — the 8 K-partials, the row's tag, the query's filter and floor: 11 registers per part — and rank_use, one MFMA chunk
    // later, sums the partials in the fixed order ((p0 + p1) + ...) + p7, filters and inserts.  Written as one function with a
    // short-circuit predicate this compiled to three DEPENDENT LDS round trips behind two exec-mask branches (tag, then
    // filter, then partials and floor) after a chunk's last MFMA, in all 8 waves at once; the predicate is bitwise now, so
    // nothing but insert_candidates' loop branches.  Every part has its own registers: at small CH two parts share a slot.
    struct RankIn {
        float pz[kWaves];
        int tag, qfilt;
        float floor;
    };
    [[maybe_unused]] RankIn RI[NT];
    auto rank_load = [&](int buf, int pq) {
#ifndef RASS_SCAN_PAIR_NORANK  // the timing-only build of the go / no-go experiment (profiles/r05_scan_pair_experiment.txt)
        const float* P = lds + buf * (kWaves * NQ * kPitch);
        const int r = lane & 31;
        const int q = pq * 16 + (lane >> 5) * 8 + wid;
        const float* src = P + q * kPitch + r;
#pragma unroll
        for (int wv = 0; wv < kWaves; ++wv) RI[pq].pz[wv] = src[wv * NQ * kPitch];
        RI[pq].tag = sh_tags[buf][r];
        RI[pq].qfilt = sh_qfilt[q];
        RI[pq].floor = sh_floor[q];
#endif
    };
    auto rank_use = [&](const WorkItem& w, int pq) {
#ifndef RASS_SCAN_PAIR_NORANK
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
#endif
    };

    // Main loop.  Iteration i multiplies tile i's two blocks and ranks tile i-1 out of the image iteration i-1 dumped: 4 parts
    // over the 2 x CH chunk slots, a part's reads ahead of its slot's MFMAs and its sum / filter / insertion behind them.  The
    // image was completed at the previous iteration's barrier, so any slot from 0 on may read it: the parts sit EARLY (slots
    // 1, 5, 9, 13 at CH = 8), which leaves no ranking between the last chunk and the barrier, where an insertion would hold up
    // all 8 waves, and — where there are slots to choose from — none in chunk 0, whose MFMAs carry the loop-top work.  One
    // barrier per iteration: it orders this iteration's dumps before the next iteration's reads, and the next iteration's
    // dumps (into the image read now) behind this iteration's reads.
    auto slot_of = [](int part) { return (part * 2 * CH) / NT + (2 * CH > NT ? 1 : 0); };
    WorkItem Pw{0, 0, 0u};  // the previous tile (rows = 0: nothing ranks in the first iteration)
    int cur = 0;            // which LDS image this iteration dumps into
    while (t < n_tiles) {
        f32x4 acc[NT];
        if (wid == 0 && lane < 32) sh_tags[cur][lane] = tag;
        const WorkItem Wc = W0;
        t = seq.next();
        const WorkItem Wn = get_work<kFlat>(p, t, n_tiles);
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
    }
    // the last tile
#pragma unroll
    for (int pq = 0; pq < NT; ++pq) {
        rank_load(cur ^ 1, pq);
        rank_use(Pw, pq);
    }
#ifdef RASS_SCAN_PAIR_NORANK
    L[0].s = lds[threadIdx.x];  // keeps the dumps alive
#endif

    // Per-workgroup sorted lists -> [gridDim.x][32][k] of each of the two groups
    const int lpos = lane & 31;
#pragma unroll
    for (int pq = 0; pq < NT; ++pq) {
        const int ql = (pq & 1) * 16 + (lane >> 5) * 8 + wid;
        if (lpos < p.k) {
            const int64_t o = (int64_t)(pq >> 1) * p.part_group_stride + ((int64_t)bid * 32 + ql) * p.k + lpos;
            const bool filled = L[pq].i != 0x7fffffff;
            p.part_scores[o] = filled ? L[pq].s : -INFINITY;
            p.part_ids[o] = filled ? (p.id_base + (int64_t)L[pq].i) : (int64_t)-1;
        }
    }
}

// ------------------------------------------------------------------------------------------
// Wide rows: 1 024 < dim <= 2 048 (row_stride = 256 * {5..8}).  EMBED_DIM is an environment knob of the reference
// (app/main.py:80) and the encoder serves hidden sizes up to 2 048, so the index must take what the encoder emits.
// A wave's K slice (row_stride / 8 columns) no longer fits its registers as one tile image, so it is walked in P
// PANELS of CHP chunks (P = 2 up to 1 792 columns, P = 4 x 4 chunks at 2 048): the two register images R0 / R1 hold
// panels pn and pn + 1 of the current tile; a panel's MFMAs continue the accumulators of the panel before it (the
// fmaf chain of the slice runs on in k order: a score is the same fixed sequence the oracle's emulation restates for
// this stride), and each consumed register is refilled with the panel TWO steps ahead in the (tile, panel) sequence.
// The query fragments of all panels stay in registers (row_stride / 32 VGPRs): that is what limits this kernel to 16
// queries per launch (NT = 1; a 32-query group runs as two launches, api_scan.hip).  Flat scans only (no IVF plan, no
// cross-index work list, no sample floor: with <= 16 queries the scan is HBM-bound and the ranking hides under it).
// Everything else — descriptors, XCD-aware item order, LDS images, one barrier per tile pair, ranking of the previous
// pair between the MFMA chunks, register-only insertion, EXT filters / continuation bound — is the kernel above.
template <int PN, int P, int CHP, typename Rank>
__device__ __forceinline__ void wide_panels(TileRegs<CHP>& R0, TileRegs<CHP>& R1, const f32x4 (&qf)[P][1][CHP],
                                            f32x4 (&acc)[2][1], const TileDesc& dcur, const TileDesc& dnext,
                                            int voff_lane, int mt_step, Rank&& rank) {
    if constexpr (PN < P) {
        constexpr bool to_next = PN + 2 >= P;                      // the refill target lies in the next tile
        constexpr int target = to_next ? PN + 2 - P : PN + 2;      // ... and is this panel of it
        multiply_and_refill<CHP, 1, to_next && target == 0, PN == 0>(
            (PN & 1) ? R1 : R0, qf[PN], acc, to_next ? dnext : dcur, voff_lane, mt_step,
            [&](int j) { if (PN == P - 1 && j == CHP - 1) rank(); }, target * CHP * 1024);
        wide_panels<PN + 1, P, CHP>(R0, R1, qf, acc, dcur, dnext, voff_lane, mt_step, rank);
    }
}

// PK: the number of panels P, plus kWideKeys where GROUP / COUNT take the row's group from its key column (the emission of
// kGroupMaxKeys / kGroupCountKeys; no bitmap on wide rows).  The flag rides in the panel slot because a template parameter
// of its own would rename every instantiation this kernel already has.
constexpr int kWideKeys = 8;
template <int CHP, int PK, bool EXT, bool RANGE, bool GROUP, bool COUNT>
__global__ __launch_bounds__(kThreads, 2) void scan_topk_f32_wide_kernel(ScanArgs p) {
    constexpr int P = PK & (kWideKeys - 1);
    constexpr bool KEYS = (PK & kWideKeys) != 0;
    static_assert((int)RANGE + (int)GROUP + (int)COUNT <= 1, "one emission per kernel");
    static_assert(!KEYS || GROUP || COUNT, "a key column feeds the grouped emissions only");
    static_assert(P == 2 || P == 4, "R0 holds the even panels, R1 the odd ones");
    constexpr int NQ = 16, CHT = P * CHP;
    extern __shared__ __attribute__((aligned(16))) float lds[];  // [4][kWaves][NQ][kPitch]
    const int lane = lane_id();
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = lane & 15, g = lane >> 4;
    if (p.live_nq != nullptr && __builtin_amdgcn_readfirstlane(*p.live_nq) == 0) return;
    const int n_tiles = (p.n_rows + kTileRows - 1) / kTileRows;
    const int G = gridDim.x;

    f32x4 qf[P][1][CHP];  // [panel]: lane (n = m, g) holds Qn[n][slice + 16 (panel CHP + j) + 4g .. +3]
    {
        const float* qbase = p.q_padded + (int64_t)m * p.row_stride + wid * 16 * CHT + 4 * g;
#pragma unroll
        for (int pn = 0; pn < P; ++pn)
#pragma unroll
            for (int j = 0; j < CHP; ++j) qf[pn][0][j] = *reinterpret_cast<const f32x4*>(qbase + 16 * (pn * CHP + j));
    }
    const int voff_lane = wid * CHT * 1024 + lane * 16;

    TopList L;
    L.s = -INFINITY;
    L.i = 0x7fffffff;
    float tau = -INFINITY;
    __shared__ int sh_qfilt[16];
    __shared__ int sh_tags[4][32];
    __shared__ int sh_qmask[16];
    __shared__ float sh_after_s[16];
    __shared__ int64_t sh_after_i[16];
    __shared__ float sh_thr[16];    // RANGE, COUNT: the per-query score thresholds (NaN past nq: nothing matches)
    __shared__ int sh_keys[4][32];  // KEYS: the dumped tiles' group keys, next to their tags
    if (threadIdx.x < 16) {
        const int q = threadIdx.x;
        const bool live = q < p.nq;
        sh_qfilt[q] = (p.q_filter != nullptr && live) ? p.q_filter[q] : -1;
        if (RANGE || COUNT) sh_thr[q] = live ? p.range_thr[q] : __builtin_nanf("");
        if (EXT) {
            sh_qmask[q] = (p.q_filter_mask != nullptr && live) ? p.q_filter_mask[q] : -1;
            sh_after_s[q] = (p.q_after_score != nullptr && live) ? p.q_after_score[q] : INFINITY;
            sh_after_i[q] = (p.q_after_id != nullptr && live) ? p.q_after_id[q] : (int64_t)-1;
        }
    }
    __syncthreads();

    const int mt_step = 16 * (int)p.row_stride * 4;
    TileRegs<CHP> R0, R1;
    ItemSeq seq((int)blockIdx.x, G, (G & 1) ? 0 : p.xcd_skew);
    int t = seq.next();
    WorkItem W0 = get_work<kFlat>(p, t, n_tiles);
    TileDesc D0 = make_tile_desc(p.corpus, p.row_stride, p.row_tag, W0);
    // KEYS: the group keys of the tile whose first panels are on their way, requested ahead of them (see scan_topk_f32_kernel)
    int K0 = 0;
    if (KEYS) K0 = load_tile_keys(p.group_keys, p.group_key_rows, W0);
    issue_tile_loads<CHP, true>(R0, D0, voff_lane, mt_step, 0);
    issue_tile_loads<CHP, false>(R1, D0, voff_lane, mt_step, CHP * 1024);
    __builtin_amdgcn_sched_barrier(0);

    auto dump_tile = [&](const f32x4 (&acc)[2][1], int buf) {
        float* P_ = lds + buf * (kWaves * NQ * kPitch);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) *reinterpret_cast<f32x4*>(P_ + (wid * NQ + m) * kPitch + mt * 16 + 4 * g) = acc[mt][0];
    };
    // wave wid ranks queries wid and 8 + wid (the two halves of the wave) of a dumped tile
    auto rank_tile = [&](const WorkItem& w, int buf) {
        const float* P_ = lds + buf * (kWaves * NQ * kPitch);
        const int r = lane & 31;
        const int row = w.tile * kTileRows + r;
        const int tag = sh_tags[buf][r];
        const bool row_ok = (r < w.rows) && (tag != -1);
        const int q = (lane >> 5) * 8 + wid;
        const int qf1 = sh_qfilt[q];
        const float* src = P_ + q * kPitch + r;
        float s = src[0];
#pragma unroll
        for (int wv = 1; wv < kWaves; ++wv) s += src[wv * NQ * kPitch];
        bool ok;
        if (EXT) {
            ok = row_ok && (qf1 < 0 || qf1 == (tag & sh_qmask[q]));
            const float as = sh_after_s[q];
            ok = ok && (s < as || (s == as && (p.id_base + (int64_t)row) > sh_after_i[q]));
        } else {
            ok = row_ok && (qf1 < 0 || qf1 == tag);
        }
        if (RANGE) {   // the emission of scan_topk_f32_kernel's kRange mode
            emit_range(ok && s >= sh_thr[q], s, row, p.range_count + q * kRangeCountStride, p.range_hits + (int64_t)q * p.range_cap,
                       p.range_cap);
            return;
        }
        if (KEYS) {   // the emission of scan_topk_f32_kernel's kGroupMaxKeys / kGroupCountKeys modes
            const int key = sh_keys[buf][r];
            ok = ok && key >= 0 && row < p.group_key_rows;
            if (GROUP)
                emit_group_max(ok && q < p.nq, s, row, key, 0x7fffffff, 0, p.group_n, p.group_table + (int64_t)q * p.group_n,
                               p.group_status);
            else
                emit_group_count(ok && s >= sh_thr[q], s, row, key, q, 0x7fffffff, 0, p.group_n, p.group_table, p.count_table,
                                 p.group_status);
            return;
        }
        if (GROUP) {   // the emission of scan_topk_f32_kernel's kGroupMax mode
            emit_group_max(ok && q < p.nq, s, row, tag, p.group_mask, p.group_shift, p.group_n,
                           p.group_table + (int64_t)q * p.group_n, p.group_status);
            return;
        }
        if (COUNT) {   // the emission of scan_topk_f32_kernel's kGroupCount mode
            emit_group_count(ok && s >= sh_thr[q], s, row, tag, q, p.group_mask, p.group_shift, p.group_n, p.group_table, p.count_table,
                             p.group_status);
            return;
        }
        s = ok ? s : -INFINITY;
        insert_candidates(L, tau, s, row, p.k);
    };

    WorkItem Pa{0, 0, 0u}, Pb{0, 0, 0u};
    int pair = 0;
    while (t < n_tiles) {
        f32x4 acc[2][1];
        // ---- tile A = W0 (its first two panels resident); the registers run on into tile B
        if (wid == 0 && lane < 32) sh_tags[pair][lane] = R0.tag;
        if (KEYS && wid == 0 && lane < 32) sh_keys[pair][lane] = K0;
        const WorkItem Wa = W0;
        const int tb = seq.next();
        const WorkItem Wb = get_work<kFlat>(p, tb, n_tiles);
        if (KEYS) K0 = load_tile_keys(p.group_keys, p.group_key_rows, Wb);
        const TileDesc Db = make_tile_desc(p.corpus, p.row_stride, p.row_tag, Wb);
        wide_panels<0, P, CHP>(R0, R1, qf, acc, D0, Db, voff_lane, mt_step, [&]() { rank_tile(Pa, pair ^ 2); });
        dump_tile(acc, pair);
        // ---- tile B; the registers run on into tile C
        if (wid == 0 && lane < 32) sh_tags[pair + 1][lane] = R0.tag;
        if (KEYS && wid == 0 && lane < 32) sh_keys[pair + 1][lane] = K0;
        t = seq.next();
        const WorkItem Wc = get_work<kFlat>(p, t, n_tiles);
        if (KEYS) K0 = load_tile_keys(p.group_keys, p.group_key_rows, Wc);
        D0 = make_tile_desc(p.corpus, p.row_stride, p.row_tag, Wc);
        wide_panels<0, P, CHP>(R0, R1, qf, acc, Db, D0, voff_lane, mt_step, [&]() { rank_tile(Pb, (pair ^ 2) + 1); });
        dump_tile(acc, pair + 1);
        W0 = Wc;
        Pa = Wa;
        Pb = Wb;
        __syncthreads();
        pair ^= 2;
    }
    rank_tile(Pa, pair ^ 2);
    rank_tile(Pb, (pair ^ 2) + 1);
    if (RANGE || GROUP || COUNT) return;

    const int lpos = lane & 31;
    const int q = (lane >> 5) * 8 + wid;
    if (q < p.nq && lpos < p.k) {
        const int64_t o = ((int64_t)blockIdx.x * p.nq + q) * p.k + lpos;
        const bool filled = L.i != 0x7fffffff;
        p.part_scores[o] = filled ? L.s : -INFINITY;
        p.part_ids[o] = filled ? (p.id_base + (int64_t)L.i) : (int64_t)-1;
    }
}

template <int CHP, int P, bool EXT, bool RANGE, bool GROUP, bool COUNT>   // P: panels (+ kWideKeys)
static hipError_t launch_wide_variant(const ScanArgs& a, int grid, hipStream_t stream) {
    constexpr size_t lds_bytes = (size_t)4 * kWaves * 16 * kPitch * sizeof(float);  // 72 KiB
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&scan_topk_f32_wide_kernel<CHP, P, EXT, RANGE, GROUP, COUNT>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    hipLaunchKernelGGL((scan_topk_f32_wide_kernel<CHP, P, EXT, RANGE, GROUP, COUNT>), dim3(grid), dim3(kThreads), lds_bytes, stream, a);
    return hipGetLastError();
}

template <bool EXT, bool RANGE = false, bool GROUP = false, bool COUNT = false, int KEYS = 0>   // KEYS: 0 or kWideKeys
static hipError_t launch_wide(int ch_total, const ScanArgs& a, int grid, hipStream_t stream) {
    switch (ch_total) {
        case 10: return launch_wide_variant<5, 2 + KEYS, EXT, RANGE, GROUP, COUNT>(a, grid, stream);
        case 12: return launch_wide_variant<6, 2 + KEYS, EXT, RANGE, GROUP, COUNT>(a, grid, stream);
        case 14: return launch_wide_variant<7, 2 + KEYS, EXT, RANGE, GROUP, COUNT>(a, grid, stream);
        case 16: return launch_wide_variant<4, 4 + KEYS, EXT, RANGE, GROUP, COUNT>(a, grid, stream);   // 2 x 8 chunks spill (256 VGPRs at 2 waves per SIMD)
        default: return hipErrorInvalidValue;
    }
}

template <int CH, int NT, int MODE, bool EXT>
static hipError_t launch_variant(const ScanArgs& a, int grid, hipStream_t stream) {
    constexpr size_t lds_bytes = (size_t)4 * kWaves * NT * 16 * kPitch * sizeof(float);  // 144 KiB at NT = 2
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&scan_topk_f32_kernel<CH, NT, MODE, EXT>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    hipLaunchKernelGGL((scan_topk_f32_kernel<CH, NT, MODE, EXT>), dim3(grid), dim3(kThreads), lds_bytes, stream, a);
    return hipGetLastError();
}

template <int NT, int MODE, bool EXT = false>
static hipError_t launch_ch(int ch, const ScanArgs& a, int grid, hipStream_t stream) {
    switch (ch) {
        case 1: return launch_variant<1, NT, MODE, EXT>(a, grid, stream);
        case 2: return launch_variant<2, NT, MODE, EXT>(a, grid, stream);
        case 3: return launch_variant<3, NT, MODE, EXT>(a, grid, stream);
        case 4: return launch_variant<4, NT, MODE, EXT>(a, grid, stream);
        case 5: return launch_variant<5, NT, MODE, EXT>(a, grid, stream);
        case 6: return launch_variant<6, NT, MODE, EXT>(a, grid, stream);
        case 7: return launch_variant<7, NT, MODE, EXT>(a, grid, stream);
        case 8: return launch_variant<8, NT, MODE, EXT>(a, grid, stream);
        default: return hipErrorInvalidValue;
    }
}

template <int CH>
static hipError_t launch_pair_variant(const ScanArgs& a, int grid, hipStream_t stream) {
    constexpr size_t lds_bytes = (size_t)2 * kWaves * 64 * kPitch * sizeof(float);  // 144 KiB
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&scan_topk_f32_pair_kernel<CH>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    hipLaunchKernelGGL((scan_topk_f32_pair_kernel<CH>), dim3(grid), dim3(kThreads), lds_bytes, stream, a);
    return hipGetLastError();
}

bool scan_pair_supported_stride(int64_t row_stride) {
    return row_stride % 128 == 0 && row_stride >= 128 && row_stride <= 1024;  // every CH compiles without scratch
}

hipError_t launch_scan_topk_f32_pair(const ScanArgs& a, int grid, hipStream_t stream) {
    if (!scan_pair_supported_stride(a.row_stride)) return hipErrorInvalidValue;
    if (a.nq != 64 || a.q_group_stride <= 0 || a.part_group_stride <= 0 || grid < 1) return hipErrorInvalidValue;
    if (a.q_filter_mask || a.q_after_score || a.q_after_id || a.work_tile || a.work_base || a.sample_pass || a.live_nq ||
        a.wgs_per_group)
        return hipErrorInvalidValue;
    switch ((int)(a.row_stride / 128)) {
        case 1: return launch_pair_variant<1>(a, grid, stream);
        case 2: return launch_pair_variant<2>(a, grid, stream);
        case 3: return launch_pair_variant<3>(a, grid, stream);
        case 4: return launch_pair_variant<4>(a, grid, stream);
        case 5: return launch_pair_variant<5>(a, grid, stream);
        case 6: return launch_pair_variant<6>(a, grid, stream);
        case 7: return launch_pair_variant<7>(a, grid, stream);
        case 8: return launch_pair_variant<8>(a, grid, stream);
        default: return hipErrorInvalidValue;
    }
}

bool scan_supported_stride(int64_t row_stride) {
    if (row_stride % 128 != 0) return false;
    const int64_t ch = row_stride / 128;
    return (ch >= 1 && ch <= 8) || (ch >= 10 && ch <= 16 && ch % 2 == 0);  // wide rows: whole 256-column units
}

// The scans that emit instead of ranking (kRange, kGroupMax, kGroupCount): flat, every stride, plain or masked filters, nothing
// else.  The mode's own fields are the caller's to check.
template <int MODE>
static hipError_t launch_emit(int ch, bool ext, const ScanArgs& a, int grid, hipStream_t stream) {
    constexpr bool R = MODE == kRange, G = MODE == kGroupMax, C = MODE == kGroupCount;
    if (a.nq < 1 || a.nq > 32) return hipErrorInvalidValue;
    if (a.q_after_score || a.q_after_id || a.work_tile || a.work_base || a.sample_pass || a.sample_best || a.wgs_per_group ||
        a.live_nq)
        return hipErrorInvalidValue;
    if (a.q_filter_mask != nullptr && a.q_filter == nullptr) return hipErrorInvalidValue;
    if (ch > 8) {
        if (a.nq > 16) return hipErrorInvalidValue;   // the caller splits larger groups, as for the top-k scan
        return ext ? launch_wide<true, R, G, C>(ch, a, grid, stream) : launch_wide<false, R, G, C>(ch, a, grid, stream);
    }
    if (a.nq <= 16) return ext ? launch_ch<1, MODE, true>(ch, a, grid, stream) : launch_ch<1, MODE>(ch, a, grid, stream);
    return ext ? launch_ch<2, MODE, true>(ch, a, grid, stream) : launch_ch<2, MODE>(ch, a, grid, stream);
}

// The group-max / group-count scans over a key column (kGroupMaxKeys / kGroupCountKeys), optionally within a bitmap: one
// variant per stride and query count, always the masked-filter one (absent masks take their neutral value in LDS).
static hipError_t launch_emit_keys(int ch, const ScanArgs& a, int grid, hipStream_t stream) {
    const bool count = a.count_table != nullptr;
    if (a.nq < 1 || a.nq > 32 || !a.group_status || a.group_n < 1 || a.group_n > kGroupMaxGroups || a.group_key_rows < 0)
        return hipErrorInvalidValue;
    if (count && !a.range_thr) return hipErrorInvalidValue;
    if (a.q_after_score || a.q_after_id || a.work_tile || a.work_base || a.sample_pass || a.sample_best || a.wgs_per_group || a.live_nq)
        return hipErrorInvalidValue;
    if ((a.q_filter_mask != nullptr && a.q_filter == nullptr) || (a.q_filter != nullptr && a.row_tag == nullptr)) return hipErrorInvalidValue;
    if (a.allow != nullptr && (ch > 8 || a.allow_q_stride < 0)) return hipErrorInvalidValue;   // the bitmap: narrow rows only
    if (ch > 8) {
        if (a.nq > 16) return hipErrorInvalidValue;   // the caller splits larger groups, as for the top-k scan
        return count ? launch_wide<true, false, false, true, kWideKeys>(ch, a, grid, stream)
                     : launch_wide<true, false, true, false, kWideKeys>(ch, a, grid, stream);
    }
    if (a.nq <= 16)
        return count ? launch_ch<1, kGroupCountKeys, true>(ch, a, grid, stream) : launch_ch<1, kGroupMaxKeys, true>(ch, a, grid, stream);
    return count ? launch_ch<2, kGroupCountKeys, true>(ch, a, grid, stream) : launch_ch<2, kGroupMaxKeys, true>(ch, a, grid, stream);
}

hipError_t launch_scan_topk_f32(const ScanArgs& a, int grid, hipStream_t stream) {
    if (!scan_supported_stride(a.row_stride)) return hipErrorInvalidValue;
    const int ch = (int)(a.row_stride / 128);
    const bool ext = a.q_filter_mask || a.q_after_score || a.q_after_id;
    // a key column (it shares range_hits' slot: a range scan, range_count set, has none)
    if (a.range_count == nullptr && a.group_table != nullptr && a.group_keys != nullptr) return launch_emit_keys(ch, a, grid, stream);
    if (a.allow != nullptr) {  // the allow-list scan: narrow rows, a work list, filters and continuation bound, nothing else
        if (!a.work_tile || !a.work_rows || !a.work_mask || !a.n_work || a.work_base || ch > 8 || a.nq < 1 || a.nq > 32 || a.allow_q_stride < 0)
            return hipErrorInvalidValue;
        if (a.range_count || a.group_table || a.sample_pass || a.sample_best || a.wgs_per_group || a.live_nq) return hipErrorInvalidValue;
        if ((a.q_after_score == nullptr) != (a.q_after_id == nullptr)) return hipErrorInvalidValue;
        if (a.q_filter_mask != nullptr && a.q_filter == nullptr) return hipErrorInvalidValue;
        // one variant per stride: 32 (zero-padded) queries, EXT — absent filters and bounds take their neutral values in LDS
        return launch_ch<2, kAllow, true>(ch, a, grid, stream);
    }
    if (a.range_count != nullptr) {  // the range scan
        if (!a.range_thr || !a.range_hits || a.range_cap < 1 || a.range_cap > kRangeMaxHits) return hipErrorInvalidValue;
        return launch_emit<kRange>(ch, ext, a, grid, stream);
    }
    const bool groups_ok = a.group_table && a.group_status && a.row_tag && a.group_mask > 0 && a.group_n >= 1 &&
                           a.group_n <= kGroupMaxGroups && a.group_shift == __builtin_ctz((unsigned)a.group_mask);
    if (a.count_table != nullptr) {  // the group-count scan
        if (!groups_ok || !a.range_thr) return hipErrorInvalidValue;
        return launch_emit<kGroupCount>(ch, ext, a, grid, stream);
    }
    if (a.group_table != nullptr) {  // the group-max scan
        if (!groups_ok) return hipErrorInvalidValue;
        return launch_emit<kGroupMax>(ch, ext, a, grid, stream);
    }
    if (a.wgs_per_group > 0 && (ext || ch > 8 || a.work_base)) return hipErrorInvalidValue;
    if (a.wgs_per_group > 0 && a.work_tile != nullptr) {  // the fine scans of several IVF launch groups in one launch
        if (!a.work_rows || !a.work_mask || !a.n_work || a.nq_total < 1 || grid % a.wgs_per_group != 0 || a.xcd_skew)
            return hipErrorInvalidValue;
        if (grid / a.wgs_per_group != (a.nq_total + 31) / 32) return hipErrorInvalidValue;
        return launch_ch<2, kIvfGroups>(ch, a, grid, stream);
    }
    if (ch > 8) {  // wide rows: flat scans of <= 16 queries (the caller splits larger groups)
        if (a.sample_pass || a.sample_best || a.work_base || a.work_tile || a.nq > 16) return hipErrorInvalidValue;
        if ((a.q_after_score == nullptr) != (a.q_after_id == nullptr)) return hipErrorInvalidValue;
        if (a.q_filter_mask != nullptr && a.q_filter == nullptr) return hipErrorInvalidValue;
        return ext ? launch_wide<true>(ch, a, grid, stream) : launch_wide<false>(ch, a, grid, stream);
    }
    if (a.sample_pass && a.wgs_per_group > 0) {  // the sample passes of a batch's launch groups in one launch
        if (ext || ch > 8 || a.work_tile || a.work_base || a.nq_total < 1 || grid % a.wgs_per_group != 0 ||
            grid / a.wgs_per_group != (a.nq_total + 31) / 32 || a.wgs_per_group > kMaxSampleGroups)
            return hipErrorInvalidValue;
        return launch_ch<2, kFlatSampleGroups>(ch, a, grid, stream);
    }
    if (a.sample_pass) {  // the score-floor sample of a flat scan with > 16 queries
        if (a.work_base != nullptr || a.work_tile != nullptr || a.nq <= 16) return hipErrorInvalidValue;
        if ((a.q_after_score == nullptr) != (a.q_after_id == nullptr)) return hipErrorInvalidValue;
        if (a.q_filter_mask != nullptr && a.q_filter == nullptr) return hipErrorInvalidValue;
        return ext ? launch_ch<2, kFlatSample, true>(ch, a, grid, stream) : launch_ch<2, kFlatSample>(ch, a, grid, stream);
    }
    if (ext && a.work_base != nullptr) {  // cross-index batch with masked filters
        if (!a.work_tile || !a.work_rows || !a.work_mask || !a.n_work || !a.work_tags) return hipErrorInvalidValue;
        if (a.q_after_score || a.q_after_id) return hipErrorInvalidValue;
        if (a.q_filter_mask != nullptr && a.q_filter == nullptr) return hipErrorInvalidValue;
        if (a.nq <= 16) return launch_ch<1, kMulti, true>(ch, a, grid, stream);
        return launch_ch<2, kMulti, true>(ch, a, grid, stream);
    }
    if (ext && a.work_tile != nullptr) {  // IVF probe with masked filters (no continuation bound: ids are slab positions)
        if (!a.work_rows || !a.work_mask || !a.n_work) return hipErrorInvalidValue;
        if (a.q_after_score || a.q_after_id) return hipErrorInvalidValue;
        if (a.q_filter_mask != nullptr && a.q_filter == nullptr) return hipErrorInvalidValue;
        if (a.nq <= 16) return launch_ch<1, kIvf, true>(ch, a, grid, stream);
        return launch_ch<2, kIvf, true>(ch, a, grid, stream);
    }
    if (ext) {  // masked filters / continuation bound of a flat scan
        if ((a.q_after_score == nullptr) != (a.q_after_id == nullptr)) return hipErrorInvalidValue;
        if (a.q_filter_mask != nullptr && a.q_filter == nullptr) return hipErrorInvalidValue;
        if (a.nq <= 16) return launch_ch<1, kFlat, true>(ch, a, grid, stream);
        return launch_ch<2, kFlat, true>(ch, a, grid, stream);
    }
    if (a.work_base != nullptr) {  // cross-index batch: every item names its slab
        if (!a.work_tile || !a.work_rows || !a.work_mask || !a.n_work || !a.work_tags) return hipErrorInvalidValue;
        if (a.nq <= 16) return launch_ch<1, kMulti>(ch, a, grid, stream);
        return launch_ch<2, kMulti>(ch, a, grid, stream);
    }
    if (a.work_tile != nullptr) {  // IVF probe: iterate the plan instead of every tile
        if (!a.work_rows || !a.work_mask || !a.n_work) return hipErrorInvalidValue;
        if (a.nq <= 16) return launch_ch<1, kIvf>(ch, a, grid, stream);
        return launch_ch<2, kIvf>(ch, a, grid, stream);
    }
    if (a.wgs_per_group > 0) {  // several launch groups of 32 (padded) queries over one slab, wgs_per_group workgroups each
        if (a.nq != 32 || grid % a.wgs_per_group != 0 || a.sample_best || a.xcd_skew) return hipErrorInvalidValue;
        return launch_ch<2, kFlatGroups>(ch, a, grid, stream);
    }
    if (a.nq <= 16) return launch_ch<1, kFlat>(ch, a, grid, stream);
    return launch_ch<2, kFlat>(ch, a, grid, stream);
}

}  // namespace rass

#ifdef RASS_SCAN_DIAG
// read-and-clear the launch counters (diagnostic builds only)
extern "C" int rassdiag_read(unsigned long long* out, int n) {
    unsigned long long h[8] = {0};
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(rass::g_scan_diag), sizeof(h)) != hipSuccess) return -2;
    for (int i = 0; i < n && i < 8; ++i) out[i] = h[i];
    unsigned long long z[8] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(rass::g_scan_diag), z, sizeof(z)) != hipSuccess) return -3;
    return 0;
}
#endif
