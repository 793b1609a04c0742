// api_ivf_allow.hip — the C ABI of include/rass_engine.h: the IVF probe within a row bitmap
// rass_ivf_search_allowed_delta(_device) — filtered k-NN that stays in the IVF instead of falling back to the flat allow
// scan —, the probed lists rass_ivf_probe_lists and (next to the bitmap builders, in api_allow.hip) rass_index_allow_count.
// Host-side C++ only: the kernels are ivf_allow.hip (the bitmap in slab order, the compacted work list), allow.hip (the
// delta's plan) and scan_topk.hip (ScanMode kAllow, unchanged).  The objects and the threading rules: api_internal.h.
//
// One launch group of <= 32 queries, under eng->mu:
//   coarse + plan   ivf_coarse_plan_locked, as every probe (both the nprobe <= 32 and the threshold branch)
//   words + compact the caller's bitmap (source rows) -> slab-order words of the planned tiles, item masks narrowed, items
//                   without a query left dropped (launch_ivf_allow_words)
//   fine scan       kAllow over the slab with the compacted work list, the slab's tags and the query filters -> list 0
//   delta           where the source holds rows behind `covered`: the flat kAllow scan restricted to them -> list 1
//   merge           (score desc, source ordinal asc), then the source's caller-assigned ids, as rass_ivf_search_delta
// Limits: an fp32 slab (the bf16 and int8 scans have no bitmap mode), k <= RASS_MAX_K (one pass, no continuation), dim <=
// 1024.  A batch of nq <= RASS_MAX_DEVICE_BATCH queries runs as groups of 32 one after another: the one-launch batch form
// of the plain probe (kIvfGroups) has no bitmap form.

#include "api_internal.h"

namespace rass {
namespace host {
namespace {

// rass_ivf::d_allow_ws of one launch group.
struct IvfAllowView {
    uint32_t* slab_allow;   // [32][total_tiles]: query q's word of slab tile t at q * total_tiles + t
    int32_t* work_tile;     // the compacted work list, <= total_tiles items
    int32_t* work_rows;
    uint32_t* work_mask;
    int32_t* n_work;
    unsigned char* place_ws;
    size_t total;
};
IvfAllowView ivf_allow_layout(unsigned char* base, int64_t tiles) {
    Carver c{base};
    IvfAllowView L;
    L.slab_allow = c.take<uint32_t>((size_t)RASS_MAX_QBATCH * tiles * sizeof(uint32_t));
    L.work_tile = c.take<int32_t>((size_t)tiles * sizeof(int32_t));
    L.work_rows = c.take<int32_t>((size_t)tiles * sizeof(int32_t));
    L.work_mask = c.take<uint32_t>((size_t)tiles * sizeof(uint32_t));
    L.n_work = c.take<int32_t>(sizeof(int32_t));
    L.place_ws = c.take<unsigned char>(rass::ivf_allow_workspace_bytes(tiles));
    L.total = c.off;
    return L;
}

struct IvfAllowRequest {   // device pointers of one launch group
    const float* queries = nullptr;     // [nq][dim]
    int nq = 0, k = 0, nprobe = 0;
    const uint32_t* allow = nullptr;    // query q's words at allow + q * q_stride, over SOURCE rows
    int64_t q_stride = 0;               // 0: one bitmap shared by every query
    int64_t words = 0;
    const int32_t* q_filter = nullptr;
    const int32_t* q_filter_mask = nullptr;
    float* out_scores = nullptr;        // [nq][k]
    int64_t* out_ids = nullptr;
};

// The checks that need neither the row count nor the lock.
int check_ivf_allowed(const rass_ivf* v, const rass_index* flat, int nq, int k, int nprobe, const uint32_t* allow, int n_bitmaps,
                      int64_t words, const int32_t* q_filter, const int32_t* q_filter_mask) {
    if (flat->eng != v->eng) return fail(RASS_ERR_INVALID, "the source index must live on the IVF's engine");
    if (nq < 0 || nq > RASS_MAX_DEVICE_BATCH) return fail(RASS_ERR_INVALID, "nq must be in [0, RASS_MAX_DEVICE_BATCH]");
    if (k < 1) return fail(RASS_ERR_INVALID, "k must be >= 1");
    if (nprobe < 1) return fail(RASS_ERR_INVALID, "nprobe must be >= 1");
    if (nq > 0 && !allow) return fail(RASS_ERR_INVALID, "NULL argument");
    if (nq > 0 && n_bitmaps != 1 && n_bitmaps != nq) return fail(RASS_ERR_INVALID, "n_bitmaps must be 1 (shared) or nq (one per query)");
    if (words < 0) return fail(RASS_ERR_INVALID, "words_per_bitmap is negative");
    if (q_filter_mask && !q_filter) return fail(RASS_ERR_INVALID, "q_filter_mask without q_filter");
    if (v->dtype != RASS_F32)
        return fail(RASS_ERR_UNSUPPORTED, "a probe within a bitmap needs an fp32 IVF slab (the bf16 and int8 scans have no bitmap mode)");
    if (k > RASS_MAX_K) return fail(RASS_ERR_UNSUPPORTED, "a probe within a bitmap serves k <= RASS_MAX_K (one pass): search the source index");
    if (v->stride > kNarrowStride) return fail(RASS_ERR_UNSUPPORTED, "a probe within a bitmap needs dim <= 1024");
    if (flat->dtype != RASS_F32 || flat->stride != v->stride || flat->dim != v->dim)
        return fail(RASS_ERR_UNSUPPORTED, "the source index must be the fp32 index the IVF was built from");
    return RASS_OK;
}

// The allow-list scan of `n_rows` rows of `corpus` over a work list, into the scratch's per-workgroup lists; the group's
// normalised queries (32 rows, zero-padded) are at the head of the scratch.
int allow_scan(rass_engine* eng, const float* corpus, const int32_t* row_tag, int64_t n_rows, int64_t stride, const IvfAllowRequest& r,
               const IvfPlan& plan, const uint32_t* allow, int64_t allow_q_stride, int64_t id_base, int* grid_out) {
    hipStream_t st = eng->stream;
    const ScratchView L = scratch_layout(eng->d_scratch, RASS_MAX_QBATCH, RASS_MAX_K);
    const int grid = scan_grid(plan.max_tiles, r.k, eng->n_cus);
    rass::ScanArgs a;
    a.corpus = corpus;
    a.row_tag = row_tag;
    a.q_padded = L.q_padded;
    a.q_filter = r.q_filter;
    a.q_filter_mask = r.q_filter_mask;
    a.part_scores = L.part_scores;
    a.part_ids = L.part_ids;
    a.row_stride = stride;
    a.id_base = id_base;
    a.n_rows = (int)n_rows;
    a.nq = r.nq;
    a.k = r.k;
    a.xcd_skew = scan_xcd_skew(RASS_MAX_QBATCH, grid, eng->n_cus);
    set_plan(a, plan);
    a.allow = allow;
    a.allow_q_stride = allow_q_stride;
    *grid_out = grid;
    return timed_launch(eng, st, [&] { return HIP_RC(rass::launch_scan_topk_f32(a, grid, st)); });
}

// One launch group; the caller holds eng->mu and has run check_ivf_allowed.  *v->d_scanned ends as the rows of the probe
// tiles kept + the rows of the delta tiles planned.
int ivf_allowed_group_locked(rass_ivf* v, rass_index* flat, const IvfAllowRequest& r) {
    rass_engine* eng = v->eng;
    hipStream_t st = eng->stream;
    const int nq = r.nq, k = r.k;
    // the IVF's ids are ordinals of the source as it was laid out at build time (a loaded IVF trusts its first source)
    const int64_t epoch = flat->layout_epoch.load(std::memory_order_acquire);
    if (v->src_epoch < 0) v->src_epoch = epoch;
    if (v->src_epoch != epoch)
        return fail(RASS_ERR_INVALID, "the source index was compacted after this IVF was built (its ids are stale ordinals): rebuild the IVF");
    const int64_t rows = flat->rows.load(std::memory_order_acquire);
    const int64_t covered = v->src_rows;
    if (covered > rows) return fail(RASS_ERR_INVALID, "the IVF covers more rows than the source index holds");
    const int64_t delta = rows - covered;
    if (delta > 0 && covered % 32 != 0)
        return fail(RASS_ERR_UNSUPPORTED, "an IVF with a delta must cover a multiple of 32 source rows (rass_ivf_build_prefix)");
    if (int rc = check_words(rows, r.words)) return rc;
    if (scratch_layout(nullptr, RASS_MAX_QBATCH, RASS_MAX_K).total > eng->scratch_bytes) return fail(RASS_ERR_INVALID, "scan workspace too small");
    const bool gid = flat->has_gid.load(std::memory_order_acquire);
    const int64_t tiles = v->total_tiles;
    const size_t before = v->allow_ws_bytes;
    int rc = grow_block(&v->d_allow_ws, &v->allow_ws_bytes, ivf_allow_layout(nullptr, tiles).total, st);
    if (rc != RASS_OK) return rc;
    // a fresh block: the scan's items past the end read tile 0's words, which no plan may have written yet
    if (v->allow_ws_bytes != before) HIP_TRY(hipMemsetAsync(v->d_allow_ws, 0, v->allow_ws_bytes, st));
    const IvfAllowView W = ivf_allow_layout(v->d_allow_ws, tiles);
    const ScratchView L = scratch_layout(eng->d_scratch, RASS_MAX_QBATCH, RASS_MAX_K);

    // coarse + plan; the queries stay normalised at the head of the scratch, padded to 16 or 32 rows: the allow scan reads 32
    rc = ivf_coarse_plan_locked(v, r.queries, nq, r.nprobe);
    if (rc != RASS_OK) return rc;
    if (pad_nq(nq) < RASS_MAX_QBATCH)
        HIP_TRY(rass::launch_zero_rows(L.q_padded + (int64_t)pad_nq(nq) * v->stride, v->stride, RASS_MAX_QBATCH - pad_nq(nq), st));
    // the bitmap in slab order, the work list compacted
    const bool shared = r.q_stride == 0;
    HIP_TRY(rass::launch_ivf_allow_words(v->d_work_tile, v->d_work_rows, v->d_work_mask, v->d_n_work, tiles, v->d_ids, r.allow, r.q_stride,
                                         r.words, nq, W.slab_allow, shared ? 0 : tiles, W.work_tile, W.work_rows, W.work_mask, W.n_work,
                                         v->d_scanned, W.place_ws, st));
    // list 0: the fine scan (slab positions), merged through the slab's ids
    float* ps = v->d_pair_scores;
    int64_t* pi = v->d_pair_ids;
    int grid = 0;
    const int32_t* slab_tag = (v->any_tags || r.q_filter != nullptr) ? v->d_tags : nullptr;
    rc = allow_scan(eng, v->d_slab, slab_tag, v->slab_rows, v->stride, r, IvfPlan{W.work_tile, W.work_rows, W.work_mask, W.n_work, tiles},
                    W.slab_allow, shared ? 0 : tiles, 0, &grid);
    if (rc != RASS_OK) return rc;
    HIP_TRY(rass::launch_merge_topk(L.part_scores, L.part_ids, grid, nq, k, ps, pi, st, v->d_ids));
    int n_lists = 1;
    if (delta > 0) {
        // list 1: the source's own slab from `covered` on, its tags and the bitmaps' words from there (covered % 32 == 0)
        rc = grow_block(&eng->d_allow, &eng->allow_bytes, allow_layout(nullptr, delta).total, st);
        if (rc != RASS_OK) return rc;
        const AllowView D = allow_layout(eng->d_allow, delta);
        const uint32_t* d_allow = r.allow + covered / 32;
        const bool need_tags = (flat->deleted.load(std::memory_order_acquire) > 0) || (r.q_filter != nullptr);
        HIP_TRY(rass::launch_allow_plan(d_allow, r.q_stride, nq, delta, D.work_tile, D.work_rows, D.work_mask, D.n_work, D.plan_ws, st));
        HIP_TRY(rass::launch_work_rows_add(D.work_rows, D.n_work, (delta + 31) / 32, nullptr, v->d_scanned, st));
        rc = allow_scan(eng, flat->d_rows + covered * flat->stride, need_tags ? flat->d_tags + covered : nullptr, delta, flat->stride, r,
                        IvfPlan{D.work_tile, D.work_rows, D.work_mask, D.n_work, (delta + 31) / 32}, d_allow, r.q_stride, covered, &grid);
        if (rc != RASS_OK) return rc;
        HIP_TRY(rass::launch_merge_topk(L.part_scores, L.part_ids, grid, nq, k, ps + (int64_t)nq * k, pi + (int64_t)nq * k, st));
        n_lists = 2;
    }
    HIP_TRY(rass::launch_merge_topk(ps, pi, n_lists, nq, k, r.out_scores, r.out_ids, st, gid ? flat->d_gid : nullptr));
    return RASS_OK;
}

}  // namespace
}  // namespace host
}  // namespace rass

using namespace rass::host;

extern "C" {

int rass_ivf_search_allowed_delta(rass_ivf_t* v, rass_index_t* flat, const float* queries, int nq, int k, int nprobe, const uint32_t* allow,
                                  int n_bitmaps, int64_t words_per_bitmap, const int32_t* q_filter, const int32_t* q_filter_mask,
                                  float* out_scores, int64_t* out_ids, int64_t* scanned_rows) {
    if (!v || !flat || !out_scores || !out_ids) return fail(RASS_ERR_INVALID, "NULL argument");
    if (nq > 0 && !queries) return fail(RASS_ERR_INVALID, "bad queries / nq");
    if (int rc = check_ivf_allowed(v, flat, nq, k, nprobe, allow, n_bitmaps, words_per_bitmap, q_filter, q_filter_mask)) return rc;
    if (scanned_rows) *scanned_rows = 0;
    if (nq == 0) return RASS_OK;
    rass_engine* eng = v->eng;
    const bool shared = n_bitmaps == 1;
    const int64_t words = words_per_bitmap;
    int64_t scanned_total = 0;
    const int rc = host_groups(
        // the bitmaps go through the engine's own staging block (eng->d_allow_io), as in rass_index_search_allowed; the answer
        // and the scanned rows through the slot
        eng, v->dim, queries, nq, q_filter, q_filter_mask, /*io_bytes=*/0, no_fill,
        [&](HostSlot* sl, int done, int b) -> int {
            hipStream_t st = eng->stream;
            const size_t bits_bytes = (size_t)(shared ? 1 : b) * words * sizeof(uint32_t);
            if (int grc = grow_block(&eng->d_allow_io, &eng->allow_io_bytes, std::max<size_t>(bits_bytes, 256), st)) return grc;
            uint32_t* d_bits = reinterpret_cast<uint32_t*>(eng->d_allow_io);
            if (bits_bytes)
                HIP_TRY(hipMemcpyAsync(d_bits, allow + (shared ? 0 : (int64_t)done * words), bits_bytes, hipMemcpyHostToDevice, st));
            IvfAllowRequest r;
            r.queries = eng->d_qraw, r.nq = b, r.k = k, r.nprobe = nprobe;
            r.allow = d_bits, r.q_stride = shared ? 0 : words, r.words = words;
            r.q_filter = q_filter ? eng->d_qfilter : nullptr, r.q_filter_mask = q_filter_mask ? eng->d_qmask : nullptr;
            r.out_scores = eng->d_out_scores, r.out_ids = eng->d_out_ids;
            const int grc = ivf_allowed_group_locked(v, flat, r);
            return grc != RASS_OK ? grc : slot_download(eng, sl, b, k, v->d_scanned);
        },
        [&](HostSlot* sl, int done, int b) -> int {
            memcpy(out_scores + (int64_t)done * k, sl->h_out_s, (size_t)b * k * 4);
            memcpy(out_ids + (int64_t)done * k, sl->h_out_i, (size_t)b * k * 8);
            scanned_total += *sl->h_scanned;
            return RASS_OK;
        });
    if (rc != RASS_OK) return rc;
    if (scanned_rows) *scanned_rows = scanned_total;
    return RASS_OK;
}

int rass_ivf_search_allowed_delta_device(rass_ivf_t* v, rass_index_t* flat, const float* d_queries, int nq, int k, int nprobe,
                                         const uint32_t* d_allow, int n_bitmaps, int64_t words_per_bitmap, const int32_t* d_q_filter,
                                         const int32_t* d_q_filter_mask, float* d_out_scores, int64_t* d_out_ids,
                                         int64_t* d_scanned_rows) {
    if (!v || !flat || !d_out_scores || !d_out_ids) return fail(RASS_ERR_INVALID, "NULL argument");
    if (nq > 0 && !d_queries) return fail(RASS_ERR_INVALID, "bad queries / nq");
    if (int rc = check_ivf_allowed(v, flat, nq, k, nprobe, d_allow, n_bitmaps, words_per_bitmap, d_q_filter, d_q_filter_mask)) return rc;
    rass_engine* eng = v->eng;
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    std::lock_guard<std::mutex> lk(eng->mu);
    if (d_scanned_rows) HIP_TRY(hipMemsetAsync(d_scanned_rows, 0, sizeof(int64_t), eng->stream));
    const bool shared = n_bitmaps == 1;
    for (int done = 0; done < nq; done += RASS_MAX_QBATCH) {
        IvfAllowRequest r;
        r.queries = d_queries + (int64_t)done * v->dim, r.nq = std::min(RASS_MAX_QBATCH, nq - done), r.k = k, r.nprobe = nprobe;
        r.allow = d_allow + (shared ? 0 : (int64_t)done * words_per_bitmap), r.q_stride = shared ? 0 : words_per_bitmap;
        r.words = words_per_bitmap;
        r.q_filter = d_q_filter ? d_q_filter + done : nullptr, r.q_filter_mask = d_q_filter_mask ? d_q_filter_mask + done : nullptr;
        r.out_scores = d_out_scores + (int64_t)done * k, r.out_ids = d_out_ids + (int64_t)done * k;
        rc = ivf_allowed_group_locked(v, flat, r);
        if (rc != RASS_OK) return rc;
        if (d_scanned_rows) HIP_TRY(rass::launch_work_rows_add(nullptr, nullptr, 0, v->d_scanned, d_scanned_rows, eng->stream));
    }
    return RASS_OK;
}

int rass_ivf_probe_lists(rass_ivf_t* v, const float* queries, int nq, int nprobe, int64_t* out_list_ids) {
    if (!v || !out_list_ids) return fail(RASS_ERR_INVALID, "NULL argument");
    if (nq < 0 || (nq > 0 && !queries)) return fail(RASS_ERR_INVALID, "bad queries / nq");
    if (nprobe < 1) return fail(RASS_ERR_INVALID, "nprobe must be >= 1");
    if (nprobe > RASS_MAX_K) return fail(RASS_ERR_UNSUPPORTED, "the probed lists are reported for nprobe <= RASS_MAX_K");
    rass_engine* eng = v->eng;
    const int kc = std::min(nprobe, v->nlist);   // lists the coarse stage ranks per query
    return host_groups(
        eng, v->dim, queries, nq, nullptr, nullptr, /*io_bytes=*/0, no_fill,
        [&](HostSlot* sl, int, int b) -> int {
            const int grc = ivf_coarse_plan_locked(v, eng->d_qraw, b, nprobe, /*plan=*/false);
            if (grc != RASS_OK) return grc;
            HIP_TRY(hipMemcpyAsync(sl->h_out_i, v->d_probe_ids, (size_t)b * kc * sizeof(int64_t), hipMemcpyDeviceToHost, eng->stream));
            return RASS_OK;
        },
        [&](HostSlot* sl, int done, int b) -> int {
            for (int q = 0; q < b; ++q)
                for (int j = 0; j < nprobe; ++j)
                    out_list_ids[((int64_t)done + q) * nprobe + j] = j < kc ? sl->h_out_i[(int64_t)q * kc + j] : (int64_t)-1;
            return RASS_OK;
        });
}

}  // extern "C"
