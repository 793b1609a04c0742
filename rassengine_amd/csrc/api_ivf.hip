// api_ivf.hip — the C ABI of include/rass_engine.h: the IVF index over a flat fp32 source.  Host-side C++ only; the launch
// helpers come from api_scan.hip, the objects and the threading rules from api_internal.h.  In this order:
//   build        the list plan of rass_ivf_build_prefix (host loops: the reference plan) and of rass_ivf_build_device /
//                rass_ivf_absorb (ivf_build.hip) both end in ivf_build_tail, which materialises the IVF (fp32, bf16, int8 slab)
//   persistence  rass_ivf_save / rass_ivf_load walk one section list (ivf_file_sections)
//   search       the probe of one launch group (coarse scan or threshold path and plan: ivf_coarse_plan_locked, which the probe
//                within a bitmap of api_ivf_allow.hip starts with as well; then the fine scan), the probe + flat delta, the
//                batch of many groups — one fine scan and one merge tail (ivf_fine_scan / ivf_fine_merge) — and the host API
//                on host_groups

#include <array>
#include <memory>

#include "api_internal.h"

using namespace rass::host;

extern "C" {

static void ivf_free(rass_ivf* v) {
    if (!v) return;
    for (void* p : {(void*)v->d_slab, (void*)v->d_slab_b16, (void*)v->d_slab_i8, (void*)v->d_slab_scale, (void*)v->d_cand_scores, (void*)v->d_cand_rows, (void*)v->d_tags, (void*)v->d_ids, (void*)v->d_centroids, (void*)v->d_list_tile0,
                    (void*)v->d_list_len, (void*)v->d_work_tile, (void*)v->d_work_rows, (void*)v->d_n_work,
                    (void*)v->d_work_mask, (void*)v->d_scanned, (void*)v->d_probe_scores, (void*)v->d_probe_ids,
                    (void*)v->d_tau, (void*)v->d_list_mask, (void*)v->d_pair_scores, (void*)v->d_pair_ids, (void*)v->d_batch, (void*)v->d_allow_ws})
        if (p) (void)hipFree(p);
    delete v;
}
// A half-built IVF: freed on every way out but the release into *out.
using IvfOwner = std::unique_ptr<rass_ivf, void (*)(rass_ivf*)>;

// Every device array of an IVF whose shape fields (dtype, strides, slab_rows, nlist, total_tiles) are set.  On a failure the
// caller frees what was allocated (ivf_free); *failed names the array that could not be had.
static hipError_t ivf_alloc(rass_ivf* v, const char** failed) {
    const size_t slab = (size_t)v->slab_rows, nl = (size_t)v->nlist, tiles = (size_t)v->total_tiles;
    const size_t cent_rows = (size_t)pad16(v->nlist), QK = RASS_MAX_QBATCH * RASS_MAX_K;
    const bool b16 = v->dtype == RASS_BF16, i8 = v->dtype == RASS_I8;
    const struct { const char* name; void** p; size_t bytes; } want[] = {
        {"d_slab_b16", (void**)&v->d_slab_b16, b16 ? slab * v->stride * 2 : 0}, {"d_slab", (void**)&v->d_slab, b16 ? 0 : slab * v->stride * 4},
        {"d_slab_i8", (void**)&v->d_slab_i8, i8 ? slab * v->stride_i8 : 0}, {"d_slab_scale", (void**)&v->d_slab_scale, i8 ? slab * 4 : 0},
        {"d_cand_scores", (void**)&v->d_cand_scores, i8 ? QK * 4 : 0}, {"d_cand_rows", (void**)&v->d_cand_rows, i8 ? QK * 8 : 0},
        {"d_tags", (void**)&v->d_tags, slab * 4}, {"d_ids", (void**)&v->d_ids, slab * 8}, {"d_centroids", (void**)&v->d_centroids, cent_rows * v->stride * 4},
        {"d_list_tile0", (void**)&v->d_list_tile0, nl * 4}, {"d_list_len", (void**)&v->d_list_len, nl * 4}, {"d_work_tile", (void**)&v->d_work_tile, tiles * 4},
        {"d_work_rows", (void**)&v->d_work_rows, tiles * 4}, {"d_work_mask", (void**)&v->d_work_mask, tiles * 4}, {"d_n_work", (void**)&v->d_n_work, 4},
        {"d_scanned", (void**)&v->d_scanned, 8}, {"d_probe_scores", (void**)&v->d_probe_scores, QK * 4}, {"d_probe_ids", (void**)&v->d_probe_ids, QK * 8},
        {"d_tau", (void**)&v->d_tau, RASS_MAX_QBATCH * 4}, {"d_list_mask", (void**)&v->d_list_mask, nl * 4}, {"d_pair_scores", (void**)&v->d_pair_scores, 2 * QK * 4},
        {"d_pair_ids", (void**)&v->d_pair_ids, 2 * QK * 8}};
    for (const auto& w : want)
        if (w.bytes) {
            const hipError_t e = hipMalloc(w.p, w.bytes);
            if (e != hipSuccess) return *failed = w.name, e;
        }
    return hipSuccess;
}

// The int8 copy of the fp32 slab and its row scales: a function of the slab (a build makes it, a load makes it again).
static int ivf_quantize_slab(rass_ivf* v, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(v->d_slab_i8, 0, (size_t)v->slab_rows * v->stride_i8, st));
    HIP_TRY(rass::launch_quantize_tile16_i8(v->d_slab, v->d_slab_i8, v->d_slab_scale, v->stride, v->stride_i8, 0, v->slab_rows / 16, st));
    return RASS_OK;
}

static int ivf_source_check(const rass_index* src, int nlist, rass_dtype slab_dtype) {
    if (nlist < 1 || nlist > kIvfMaxLists) return fail(RASS_ERR_INVALID, "nlist must be in [1, 32768]");
    if (src->dtype != RASS_F32) return fail(RASS_ERR_UNSUPPORTED, "the IVF build needs an fp32 source index");
    if (src->stride > kNarrowStride) return fail(RASS_ERR_UNSUPPORTED, "IVF needs dim <= 1024 (wide rows: flat scan only)");
    if (slab_dtype != RASS_F32 && slab_dtype != RASS_BF16 && slab_dtype != RASS_I8) return fail(RASS_ERR_INVALID, "unknown slab dtype");
    if (slab_dtype == RASS_BF16 && src->stride % 256 != 0)
        return fail(RASS_ERR_UNSUPPORTED, "a bf16 slab needs dim padded to a multiple of 256 (the bf16 scan's K split)");
    return RASS_OK;
}

// The list plan of a build over source rows [0, n): where every live row goes.  All four arrays on the host
// (rass_ivf_build_prefix's loops) or all four on the device (ivf_build.hip).
struct IvfListPlan {
    int64_t tiles, live;          // tiles of all lists (0: no live row, the slab is one padding tile); live rows
    const int32_t *len, *tile0;   // [nlist] live rows and first tile of every list
    const int64_t* ids;           // [max(tiles, 1) * tile_rows] source row of every slab position, -1 on padding
    const int32_t* pos_of;        // [n] slab position of every source row, -1 = in no list
    bool on_device;
};

// What every build does once its lists are planned: the IVF object and its device arrays, the list tables, the rows permuted
// into the slab (fp32 or bf16; an int8 slab quantised from the fp32 one), the tags gathered through the slab's ids (padding
// keeps 0) and the centroids — exactly one of `centroids` (host, row-major: normalised and packed through the engine's
// staging buffer) and `d_centroids_tile16` (a centroid slab of the same nlist and stride: copied).  The caller holds src->mu,
// has set the device and checked src / nlist / slab_dtype (ivf_source_check).  Returns with the stream idle.
static int ivf_build_tail(rass_index* src, int nlist, rass_dtype slab_dtype, int64_t n, const IvfListPlan& p, const float* centroids,
                          const float* d_centroids_tile16, rass_ivf_t** out) {
    rass_engine* eng = src->eng;
    hipStream_t st = eng->stream;
    IvfOwner v(new (std::nothrow) rass_ivf(), ivf_free);
    if (!v) return fail(RASS_ERR_OOM, "host allocation failed");
    v->eng = eng;
    v->dtype = slab_dtype;
    v->tile_rows = slab_dtype == RASS_F32 ? 32 : 64;
    v->dim = src->dim;
    v->stride = src->stride;
    v->nlist = nlist;
    v->rows = p.live;
    v->src_rows = n;
    v->src_epoch = src->layout_epoch.load();
    v->total_tiles = std::max<int64_t>(p.tiles, 1);
    v->slab_rows = v->total_tiles * v->tile_rows;
    v->any_tags = src->has_tags;
    if (slab_dtype == RASS_I8) v->stride_i8 = pad512(v->stride);
    try {
        v->pos_of.resize((size_t)n);
    } catch (const std::bad_alloc&) {
        return fail(RASS_ERR_OOM, "host allocation failed");
    }
    const char* what = "";
    const hipError_t ae = ivf_alloc(v.get(), &what);
    if (ae != hipSuccess)
        return fail(ae == hipErrorOutOfMemory ? RASS_ERR_OOM : RASS_ERR_HIP, std::string("ivf build: hipMalloc of ") + what + ": " + hipGetErrorString(ae));
    const size_t slab = (size_t)v->slab_rows, cent_bytes = (size_t)pad16(nlist) * v->stride * 4;
    const hipMemcpyKind to_device = p.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    HIP_TRY(hipMemcpyAsync(v->d_ids, p.ids, slab * 8, to_device, st));
    HIP_TRY(hipMemcpyAsync(v->d_list_tile0, p.tile0, (size_t)nlist * 4, to_device, st));
    HIP_TRY(hipMemcpyAsync(v->d_list_len, p.len, (size_t)nlist * 4, to_device, st));
    if (n > 0 && p.on_device) HIP_TRY(hipMemcpyAsync(v->pos_of.data(), p.pos_of, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (n > 0 && !p.on_device) memcpy(v->pos_of.data(), p.pos_of, (size_t)n * 4);
    if (slab_dtype == RASS_BF16)
        HIP_TRY(rass::launch_permute_rows_tile16_bf16(src->d_rows, v->d_slab_b16, v->stride, v->d_ids, v->slab_rows, st));
    else
        HIP_TRY(rass::launch_permute_rows_tile16(src->d_rows, v->d_slab, v->stride, v->d_ids, v->slab_rows, st));
    if (slab_dtype == RASS_I8)
        if (int rc = ivf_quantize_slab(v.get(), st)) return rc;
    HIP_TRY(hipMemsetAsync(v->d_tags, 0, slab * 4, st));
    HIP_TRY(rass::launch_gather_i32(src->d_tags, v->d_tags, v->d_ids, v->slab_rows, n, st));
    if (d_centroids_tile16) {
        HIP_TRY(hipMemcpyAsync(v->d_centroids, d_centroids_tile16, cent_bytes, hipMemcpyDeviceToDevice, st));
    } else {
        HIP_TRY(hipMemsetAsync(v->d_centroids, 0, cent_bytes, st));
        std::lock_guard<std::mutex> elk(eng->mu);
        for (int64_t done = 0; done < nlist; done += kStageRows) {
            const int64_t m = std::min<int64_t>(kStageRows, nlist - done);
            HIP_TRY(hipMemcpyAsync(eng->d_stage, centroids + done * v->dim, (size_t)m * v->dim * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(rass::launch_pack_rows_tile16(eng->d_stage, v->dim, v->d_centroids, v->stride, done, m, v->dim, 1, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
    }
    HIP_TRY(hipStreamSynchronize(st));   // the plan's arrays are the caller's: nothing reads them after the return
    *out = v.release();
    return RASS_OK;
}

int rass_ivf_build(rass_index_t* src, const float* centroids, int nlist, const int32_t* assign, rass_ivf_t** out) {
    return rass_ivf_build_ex(src, centroids, nlist, assign, RASS_F32, out);
}

int rass_ivf_build_ex(rass_index_t* src, const float* centroids, int nlist, const int32_t* assign, rass_dtype slab_dtype,
                      rass_ivf_t** out) {
    return rass_ivf_build_prefix(src, centroids, nlist, assign, slab_dtype, -1, out);
}

// The host-planned build.  Its loops over assign[] and the tombstone bitmap DEFINE the list plan: the device plan of
// ivf_build.hip is tested against them (tests/test_gpu_ivf_absorb.py compares the two builds' saved files).
int rass_ivf_build_prefix(rass_index_t* src, const float* centroids, int nlist, const int32_t* assign,
                          rass_dtype slab_dtype, int64_t n_rows, rass_ivf_t** out) {
    if (!src || !centroids || !assign || !out) return fail(RASS_ERR_INVALID, "NULL argument");
    *out = nullptr;
    int rc = ivf_source_check(src, nlist, slab_dtype);
    if (rc != RASS_OK) return rc;
    const int tile_rows = slab_dtype == RASS_F32 ? 32 : 64;
    std::lock_guard<std::mutex> lk(src->mu);
    rc = set_device(src->eng);
    if (rc != RASS_OK) return rc;
    if (n_rows > src->rows) return fail(RASS_ERR_INVALID, "n_rows exceeds the rows of the source index");
    const int64_t n = n_rows < 0 ? src->rows.load() : n_rows;
    const auto dead = [&](int64_t r) { return (src->host_deleted[(size_t)(r >> 3)] & (1u << (r & 7))) != 0; };
    // list lengths over live rows, tile-aligned offsets
    std::vector<int32_t> len((size_t)nlist, 0), tile0((size_t)nlist, 0);
    int64_t live = 0;
    for (int64_t r = 0; r < n; ++r) {
        if (dead(r)) continue;
        const int32_t l = assign[r];
        if (l < 0 || l >= nlist) return fail(RASS_ERR_INVALID, "assign[] holds a list id outside [0, nlist)");
        len[(size_t)l] += 1;
        live += 1;
    }
    int64_t tiles = 0;
    for (int l = 0; l < nlist; ++l) {
        tile0[(size_t)l] = (int32_t)tiles;
        tiles += (len[(size_t)l] + tile_rows - 1) / tile_rows;
    }
    if (tiles * tile_rows > kMaxScanRows) return fail(RASS_ERR_UNSUPPORTED, "slab too large for one IVF shard");
    std::vector<int64_t> src_of((size_t)(std::max<int64_t>(tiles, 1) * tile_rows), -1);
    std::vector<int32_t> fill((size_t)nlist, 0), pos_of((size_t)n, -1);
    for (int64_t r = 0; r < n; ++r) {  // ascending source id inside every list
        if (dead(r)) continue;
        const int32_t l = assign[r];
        const int64_t d = (int64_t)tile0[(size_t)l] * tile_rows + fill[(size_t)l]++;
        src_of[(size_t)d] = r;
        pos_of[(size_t)r] = (int32_t)d;
    }
    const IvfListPlan plan{tiles, live, len.data(), tile0.data(), src_of.data(), pos_of.data(), /*on_device=*/false};
    return ivf_build_tail(src, nlist, slab_dtype, n, plan, centroids, nullptr, out);
}

void rass_ivf_destroy(rass_ivf_t* v) {
    if (!v) return;
    (void)hipSetDevice(v->eng->device);
    (void)hipStreamSynchronize(v->eng->stream);
    ivf_free(v);
}

// ---- IVF persistence: header (+ the covered rows) + list table + slab ids + tags + centroid slab + row slab (raw tile16)
struct IvfSaveHeader {
    char magic[8];
    int32_t version, dim, nlist, any_tags;
    int64_t stride, rows, slab_rows, total_tiles, cent_rows;
};

// The device arrays behind the header, in file order; the shape fields of `v` give the sizes (the int8 copy and its scales are
// not stored: ivf_quantize_slab).
struct IvfSection {
    void* p;
    size_t bytes;
};
static std::array<IvfSection, 6> ivf_file_sections(const rass_ivf* v) {
    const size_t slab = (size_t)v->slab_rows, nl = (size_t)v->nlist, stride = (size_t)v->stride;
    return {{{v->d_list_tile0, nl * 4}, {v->d_list_len, nl * 4}, {v->d_ids, slab * 8}, {v->d_tags, slab * 4},
             {v->d_centroids, (size_t)pad16(v->nlist) * stride * 4},
             v->dtype == RASS_BF16 ? IvfSection{v->d_slab_b16, slab * stride * 2} : IvfSection{v->d_slab, slab * stride * 4}}};
}

// One section between the device and the file, through a bounce buffer.
static bool section_io(FILE* f, const IvfSection& s, bool save, hipStream_t st, std::vector<unsigned char>& buf) {
    unsigned char* p = static_cast<unsigned char*>(s.p);
    for (size_t done = 0; done < s.bytes;) {
        const size_t m = std::min(buf.size(), s.bytes - done);
        if (!save && fread(buf.data(), 1, m, f) != m) return false;
        const hipError_t e = save ? hipMemcpyAsync(buf.data(), p + done, m, hipMemcpyDeviceToHost, st)
                                  : hipMemcpyAsync(p + done, buf.data(), m, hipMemcpyHostToDevice, st);
        if (e != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return false;
        if (save && fwrite(buf.data(), 1, m, f) != m) return false;
        done += m;
    }
    return true;
}

struct FileCloser {
    void operator()(FILE* f) const { fclose(f); }
};

int rass_ivf_save(rass_ivf_t* v, const char* path) {
    if (!v || !path) return fail(RASS_ERR_INVALID, "NULL argument");
    rass_engine* eng = v->eng;
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    std::lock_guard<std::mutex> lk(eng->mu);
    hipStream_t st = eng->stream;
    FILE* f = fopen(path, "wb");
    if (!f) return fail(RASS_ERR_IO, std::string("cannot open for write: ") + path);
    IvfSaveHeader h;
    memset(&h, 0, sizeof(h));
    memcpy(h.magic, "RASSIVF1", 8);
    // 3 / 4 (since round 4) = 1 / 2 followed by one int64: the source rows the IVF covers (rass_ivf_covered_rows).
    // 2, 4: the row slab is bf16 (tile16b) with lists on 64-row tiles
    // 5: the fp32 slab with lists on 64-row tiles of an int8 IVF (the int8 copy and its scales are rebuilt by the load)
    h.version = v->dtype == RASS_BF16 ? 4 : v->dtype == RASS_I8 ? 5 : 3;
    h.dim = v->dim;
    h.nlist = v->nlist;
    h.any_tags = v->any_tags ? 1 : 0;
    h.stride = v->stride;
    h.rows = v->rows;
    h.slab_rows = v->slab_rows;
    h.total_tiles = v->total_tiles;
    h.cent_rows = pad16(v->nlist);
    std::vector<unsigned char> buf((size_t)32 << 20);
    bool ok = fwrite(&h, sizeof(h), 1, f) == 1;
    ok = ok && fwrite(&v->src_rows, sizeof(int64_t), 1, f) == 1;
    for (const IvfSection& s : ivf_file_sections(v)) ok = ok && section_io(f, s, /*save=*/true, st, buf);
    ok = ok && fflush(f) == 0 && fsync(fileno(f)) == 0;
    ok = (fclose(f) == 0) && ok;
    return ok ? RASS_OK : fail(RASS_ERR_IO, std::string("ivf save failed (short write or device read): ") + path);
}

int rass_ivf_load(rass_engine_t* eng, const char* path, rass_ivf_t** out) {
    if (!eng || !path || !out) return fail(RASS_ERR_INVALID, "NULL argument");
    *out = nullptr;
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    const std::unique_ptr<FILE, FileCloser> file(fopen(path, "rb"));
    FILE* f = file.get();
    if (!f) return fail(RASS_ERR_IO, std::string("cannot open for read: ") + path);
    IvfSaveHeader h;
    if (fread(&h, sizeof(h), 1, f) != 1 || memcmp(h.magic, "RASSIVF1", 8) != 0 || h.version < 1 || h.version > 5)
        return fail(RASS_ERR_IO, "not a rass IVF file");
    int64_t src_rows = -1;   // versions 1 / 2 do not carry it: taken from the slab's ids below
    const int64_t extra = h.version >= 3 ? (int64_t)sizeof(int64_t) : 0;
    if (extra && (fread(&src_rows, sizeof(int64_t), 1, f) != 1 || src_rows < 0)) return fail(RASS_ERR_IO, "IVF file is truncated / corrupt");
    const bool b16 = h.version == 2 || h.version == 4;
    const bool i8 = h.version == 5;
    const int tile_rows = (b16 || i8) ? 64 : 32;
    bool sane = h.dim == eng->dim && h.stride == pad128(h.dim) && h.nlist >= 1 && h.nlist <= kIvfMaxLists && h.rows >= 0 &&
                h.slab_rows >= tile_rows && h.slab_rows % tile_rows == 0 && h.slab_rows <= kMaxScanRows &&
                h.total_tiles == h.slab_rows / tile_rows && h.cent_rows == pad16(h.nlist) && h.rows <= h.slab_rows &&
                (!b16 || h.stride % 256 == 0) && h.stride <= kNarrowStride;
    IvfOwner v(sane ? new (std::nothrow) rass_ivf() : nullptr, ivf_free);
    if (sane && !v) return fail(RASS_ERR_OOM, "host allocation failed");
    if (sane) {  // the header must agree with the file length before anything is allocated from it
        v->eng = eng;
        v->dim = h.dim;
        v->stride = h.stride;
        v->nlist = h.nlist;
        v->rows = h.rows;
        v->slab_rows = h.slab_rows;
        v->total_tiles = h.total_tiles;
        v->any_tags = h.any_tags != 0;
        v->dtype = b16 ? RASS_BF16 : i8 ? RASS_I8 : RASS_F32;
        v->tile_rows = tile_rows;
        v->stride_i8 = pad512(h.stride);
        const long body = ftell(f);
        int64_t len = -1, need = (int64_t)sizeof(h) + extra;
        if (body >= 0 && fseek(f, 0, SEEK_END) == 0) len = (int64_t)ftell(f);
        for (const IvfSection& s : ivf_file_sections(v.get())) need += (int64_t)s.bytes;
        sane = body >= 0 && len == need && fseek(f, body, SEEK_SET) == 0;
    }
    if (!sane) return fail(RASS_ERR_IO, "IVF file does not match the engine (dim) or is truncated / corrupt");
    std::lock_guard<std::mutex> lk(eng->mu);
    hipStream_t st = eng->stream;
    const char* what = "";
    if (ivf_alloc(v.get(), &what) != hipSuccess) return fail(RASS_ERR_OOM, std::string("ivf load: device allocation failed (") + what + ")");
    std::vector<unsigned char> buf((size_t)32 << 20);
    bool ok = true;
    for (const IvfSection& s : ivf_file_sections(v.get())) ok = ok && section_io(f, s, /*save=*/false, st, buf);
    if (ok && i8)   // the int8 copy is a function of the fp32 slab: rebuilt, not stored
        ok = ivf_quantize_slab(v.get(), st) == RASS_OK && hipStreamSynchronize(st) == hipSuccess;
    if (!ok) return fail(RASS_ERR_IO, "ivf load: short read or upload failure");
    // the list table must index inside the slab: a corrupt table would send the probe out of bounds
    {
        std::vector<int32_t> t0((size_t)h.nlist), len((size_t)h.nlist);
        bool good = hipMemcpy(t0.data(), v->d_list_tile0, (size_t)h.nlist * 4, hipMemcpyDeviceToHost) == hipSuccess &&
                    hipMemcpy(len.data(), v->d_list_len, (size_t)h.nlist * 4, hipMemcpyDeviceToHost) == hipSuccess;
        int64_t tiles = 0;
        for (int l = 0; good && l < h.nlist; ++l) {
            good = len[(size_t)l] >= 0 && t0[(size_t)l] == tiles;
            tiles += (len[(size_t)l] + tile_rows - 1) / tile_rows;
        }
        if (!good || std::max<int64_t>(tiles, 1) != h.total_tiles) return fail(RASS_ERR_IO, "ivf load: inconsistent list table");
    }
    // source row -> slab position (rass_ivf_delete), from the slab's ids and tags (-1 tag = tombstoned after the build)
    {
        std::vector<int64_t> ids((size_t)h.slab_rows);
        std::vector<int32_t> tags((size_t)h.slab_rows);
        if (hipMemcpy(ids.data(), v->d_ids, (size_t)h.slab_rows * 8, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(tags.data(), v->d_tags, (size_t)h.slab_rows * 4, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(RASS_ERR_HIP, "ivf load: reading back the slab ids failed");
        int64_t max_id = -1;
        for (int64_t d = 0; d < h.slab_rows; ++d) max_id = std::max(max_id, ids[(size_t)d]);
        if (src_rows < 0) src_rows = max_id + 1;
        if (max_id >= src_rows) return fail(RASS_ERR_IO, "ivf load: a slab id lies outside the covered source rows");
        v->src_rows = src_rows;
        v->pos_of.assign((size_t)src_rows, -1);
        for (int64_t d = 0; d < h.slab_rows; ++d)
            if (ids[(size_t)d] >= 0 && tags[(size_t)d] != -1) v->pos_of[(size_t)ids[(size_t)d]] = (int32_t)d;
    }
    *out = v.release();
    return RASS_OK;
}

int64_t rass_ivf_rows(const rass_ivf_t* v) { return v ? v->rows : 0; }
int rass_ivf_nlist(const rass_ivf_t* v) { return v ? v->nlist : 0; }
int rass_ivf_dtype(const rass_ivf_t* v) { return v ? v->dtype : -1; }
int64_t rass_ivf_covered_rows(const rass_ivf_t* v) { return v ? v->src_rows : 0; }

int rass_ivf_delete(rass_ivf_t* v, int64_t src_row) {
    if (!v) return fail(RASS_ERR_INVALID, "NULL argument");
    rass_engine* eng = v->eng;
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    // the engine mutex: a search holds it for its whole enqueue sequence, so the fill cannot land between a probe's
    // plan and its fine scan (as rass_index_delete)
    std::lock_guard<std::mutex> lk(eng->mu);
    if (src_row < 0 || src_row >= v->src_rows) return RASS_OK;   // not covered: the row lives in the flat delta only
    const int32_t pos = v->pos_of[(size_t)src_row];
    if (pos < 0) return RASS_OK;                                  // already gone
    const int32_t dead = -1;
    HIP_TRY(hipMemcpyAsync(v->d_tags + pos, &dead, 4, hipMemcpyHostToDevice, eng->stream));
    HIP_TRY(hipStreamSynchronize(eng->stream));                   // `dead` is a stack variable
    v->pos_of[(size_t)src_row] = -1;
    v->any_tags = true;
    v->rows -= 1;
    return RASS_OK;
}

// The centroid slab as the corpus of the exact fp32 scan: `nq` normalised queries at q_padded, k centroids per query and
// workgroup into the lists at part_scores / part_ids.  (The probe of <= 32 lists goes through scan_launch instead.)
static rass::ScanArgs ivf_centroid_args(const rass_ivf* v, const float* q_padded, float* part_scores, int64_t* part_ids, int nq, int k) {
    rass::ScanArgs a;
    a.corpus = v->d_centroids;
    a.row_tag = nullptr;
    a.q_padded = q_padded;
    a.q_filter = nullptr;
    a.part_scores = part_scores;
    a.part_ids = part_ids;
    a.row_stride = v->stride;
    a.id_base = 0;
    a.n_rows = v->nlist;
    a.nq = nq;
    a.k = k;
    return a;
}

// One launch group of a fine scan: its queries normalised at v->stride (q_f32: the fp32 scan and the int8 re-rank) and, for
// a bf16 / int8 slab, converted (q_low); its filters; the per-workgroup lists it writes.
struct IvfGroup {
    const float* q_f32;
    const void* q_low;
    const int32_t *q_filter, *q_filter_mask;
    float* part_scores;
    int64_t* part_ids;
    int nq;
};

// The fp32 slab as the corpus of the exact scan, for group g; the caller adds the work list.
static rass::ScanArgs ivf_f32_args(const rass_ivf* v, const int32_t* row_tag, const IvfGroup& g, int k) {
    rass::ScanArgs a;
    a.corpus = v->d_slab;
    a.row_tag = row_tag;
    a.q_padded = g.q_f32;
    a.q_filter = g.q_filter;
    a.q_filter_mask = g.q_filter_mask;
    a.part_scores = g.part_scores;
    a.part_ids = g.part_ids;
    a.row_stride = v->stride;
    a.id_base = 0;
    a.n_rows = (int)v->slab_rows;
    a.nq = g.nq;
    a.k = k;
    return a;
}

// The fine scan of one launch group over the slab, whatever its dtype: `grid` workgroups over the planned tiles, k entries per
// query and workgroup (slab positions), under the engine's kernel timing.
static int ivf_fine_scan(rass_ivf* v, const int32_t* row_tag, const IvfGroup& g, int k, const IvfPlan& plan, int grid) {
    hipStream_t st = v->eng->stream;
    return timed_launch(v->eng, st, [&] {
        if (v->dtype == RASS_BF16) {
            rass::ScanBf16Args a = bf16_args(v, row_tag, k);
            set_group(a, g.q_low, g.q_filter, g.q_filter_mask, g.part_scores, g.part_ids, g.nq);
            set_plan(a, plan);
            return HIP_RC(rass::launch_scan_bf16_topk(a, grid, st));
        }
        if (v->dtype == RASS_I8) {
            rass::ScanI8Args a = i8_args(v, row_tag, k);
            set_group(a, g.q_low, g.q_filter, g.q_filter_mask, g.part_scores, g.part_ids, g.nq);
            set_plan(a, plan);
            return HIP_RC(rass::launch_scan_i8_topk(a, grid, st));
        }
        rass::ScanArgs a = ivf_f32_args(v, row_tag, g, k);
        set_plan(a, plan);
        return HIP_RC(rass::launch_scan_topk_f32(a, grid, st));
    });
}

// The fine lists of `grid` workgroups (per group, where `groups` says so) -> the answer: merged, slab positions -> source ids.
// An int8 slab's lists hold 32 candidates per query: merged to cand_scores / cand_rows, then rescored exactly from the fp32 slab
// in the flat kernel's order, the best k under (score desc, source id asc) reported.
static int ivf_fine_merge(rass_ivf* v, const float* part_scores, const int64_t* part_ids, int grid, int nq, int k, const float* q_f32,
                          float* cand_scores, int64_t* cand_rows, const rass::MergeGroups* groups, float* d_out_scores,
                          int64_t* d_out_ids) {
    hipStream_t st = v->eng->stream;
    if (v->dtype != RASS_I8) {
        HIP_TRY(rass::launch_merge_topk(part_scores, part_ids, grid, nq, k, d_out_scores, d_out_ids, st, v->d_ids, 0, 0, groups));
        return RASS_OK;
    }
    HIP_TRY(rass::launch_merge_topk(part_scores, part_ids, grid, nq, RASS_MAX_K, cand_scores, cand_rows, st, nullptr, 0, 0, groups));
    HIP_TRY(rass::launch_rerank_f32(v->d_slab, v->stride, q_f32, cand_rows, nq, RASS_MAX_K, k, 0, d_out_scores, d_out_ids, st, 0, 0, v->d_ids));
    return RASS_OK;
}

constexpr const char* kIvfI8MaxKMsg = "an int8 IVF slab serves k <= 16 (32 candidates per query)";

}  // extern "C"

// The coarse stage and the plan of one launch group (declared in api_internal.h: the probe within a row bitmap starts the same way).
int rass::host::ivf_coarse_plan_locked(rass_ivf* v, const float* d_queries, int nq, int nprobe, bool plan) {
    if (!v || !d_queries) return fail(RASS_ERR_INVALID, "NULL argument");
    if (nprobe < 1) return fail(RASS_ERR_INVALID, "nprobe must be >= 1");
    if (int rc = check_nq(nq)) return rc;
    rass_engine* eng = v->eng;
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    hipStream_t st = eng->stream;
    const int np = std::min(nprobe, v->nlist);
    const int n_ctiles = (v->nlist + 31) / 32;
    if (!plan && np > RASS_MAX_K) return fail(RASS_ERR_UNSUPPORTED, "the probed lists are reported for nprobe <= RASS_MAX_K");
    if (np <= RASS_MAX_K || n_ctiles > kMaxGrid) {
        // (i) coarse: top-nprobe centroids per query with the flat fused scan
        ScanRequest c = scan_request(eng);
        c.stride = v->stride, c.queries = d_queries, c.q_dim = v->dim, c.q_stride = v->dim, c.nq = nq;
        c.corpus = v->d_centroids, c.n_rows = v->nlist, c.k = std::min(np, RASS_MAX_K);
        c.out_scores = v->d_probe_scores, c.out_ids = v->d_probe_ids;
        rc = scan_launch(c);
        if (rc != RASS_OK || !plan) return rc;
        // (ii) plan: union of probed lists -> work tiles with per-tile query masks
        HIP_TRY(rass::launch_plan_probe(v->d_probe_ids, nq, std::min(np, RASS_MAX_K), v->nlist, v->d_list_tile0,
                                        v->d_list_len, v->d_work_tile, v->d_work_rows, v->d_work_mask, v->d_n_work,
                                        v->d_scanned, st, nullptr, v->tile_rows));
    } else {
        // nprobe > 32: one workgroup per 32-centroid tile with k = 32 leaves EVERY centroid score in
        // the per-workgroup lists; radix-select the nprobe-th best per query, mask by threshold
        const ScratchView L = scratch_layout(eng->d_scratch, nq, RASS_MAX_K);
        HIP_TRY(rass::launch_normalize_rows_f32(d_queries, v->dim, L.q_padded, v->stride, nq, v->dim, st, pad_nq(nq)));
        const rass::ScanArgs a = ivf_centroid_args(v, L.q_padded, L.part_scores, L.part_ids, nq, RASS_MAX_K);
        HIP_TRY(rass::launch_scan_topk_f32(a, n_ctiles, st));
        HIP_TRY(rass::launch_ivf_threshold(L.part_scores, L.part_ids, n_ctiles, nq, np, v->d_tau, st));
        HIP_TRY(rass::launch_ivf_mask_from_scores(L.part_scores, L.part_ids, n_ctiles, nq, v->nlist, v->d_tau,
                                                  v->d_list_mask, st));
        HIP_TRY(rass::launch_plan_probe(v->d_probe_ids, nq, 1, v->nlist, v->d_list_tile0, v->d_list_len, v->d_work_tile,
                                        v->d_work_rows, v->d_work_mask, v->d_n_work, v->d_scanned, st, v->d_list_mask,
                                        v->tile_rows));
    }
    return RASS_OK;
}

extern "C" {

// Caller holds eng->mu (the probe scratch of the IVF object and the engine scratch are shared).
static int ivf_search_locked(rass_ivf_t* v, const float* d_queries, int nq, int k, int nprobe, const int32_t* d_q_filter,
                             const int32_t* d_q_filter_mask, float* d_out_scores, int64_t* d_out_ids) {
    if (!v || !d_queries || !d_out_scores || !d_out_ids) return fail(RASS_ERR_INVALID, "NULL argument");
    int rc = ivf_coarse_plan_locked(v, d_queries, nq, nprobe);
    if (rc != RASS_OK) return rc;
    rass_engine* eng = v->eng;
    hipStream_t st = eng->stream;
    // what the fine scan takes over from the coarse one: the caller's queries, one launch group, the engine's scratch and stream
    ScanRequest s = scan_request(eng);
    s.stride = v->stride, s.queries = d_queries, s.q_dim = v->dim, s.q_stride = v->dim, s.nq = nq;
    // (iii) fine: the same fused scan over the planned tiles; slab positions -> source ids in the merge
    const IvfPlan plan{v->d_work_tile, v->d_work_rows, v->d_work_mask, v->d_n_work, v->total_tiles};
    const int32_t* row_tag = (v->any_tags || d_q_filter != nullptr) ? v->d_tags : nullptr;
    // (both branches above left the batch's normalised queries at the head of the engine scratch, at this stride)
    if (v->dtype == RASS_F32) {
        s.corpus = v->d_slab, s.n_rows = v->slab_rows, s.row_tag = row_tag, s.q_filter = d_q_filter, s.k = k;
        s.out_scores = d_out_scores, s.out_ids = d_out_ids, s.timing = eng, s.plan = &plan, s.id_map = v->d_ids;
        s.ext.d_q_mask = d_q_filter_mask;
        s.queries_prepared = true;
        return scan_launch(s);
    }
    // a bf16 slab: queries rounded to bf16, fp32 accumulation over the planned 64-row tiles — the scores of a flat bf16 index
    // holding the same rows.  An int8 slab: the scan keeps 32 candidates per query whatever k is (ivf_fine_merge).
    const ScratchView L = scratch_layout(eng->d_scratch, RASS_MAX_QBATCH, RASS_MAX_K);
    const bool i8 = v->dtype == RASS_I8;
    if (i8 && k > kPrefilterMaxK) return fail(RASS_ERR_UNSUPPORTED, kIvfI8MaxKMsg);
    const int kf = i8 ? RASS_MAX_K : k;
    if (i8) HIP_TRY(rass::launch_queries_to_i8(L.q_padded, L.q_bf16, pad_nq(nq), v->stride, v->stride_i8, st));
    else HIP_TRY(rass::launch_queries_to_bf16(L.q_padded, L.q_bf16, (int64_t)pad_nq(nq) * v->stride, st));
    const int grid = scan_grid(v->total_tiles, kf, eng->n_cus);
    const IvfGroup g{L.q_padded, L.q_bf16, d_q_filter, d_q_filter_mask, L.part_scores, L.part_ids, nq};
    rc = ivf_fine_scan(v, row_tag, g, kf, plan, grid);
    if (rc != RASS_OK) return rc;
    return ivf_fine_merge(v, L.part_scores, L.part_ids, grid, nq, k, L.q_padded, v->d_cand_scores, v->d_cand_rows, nullptr, d_out_scores,
                          d_out_ids);
}

// One launch group of an IVF + delta search; the caller holds eng->mu.  List 0 = the probe (source ordinals through the
// slab's id map), list 1 = the exact scan of the source rows the IVF does not cover (ordinals through id_base); the
// final merge orders them by (score desc, ordinal asc) and maps ordinals to the source's caller-assigned ids, if any.
static int ivf_delta_group_locked(rass_ivf_t* v, rass_index* flat, const float* d_queries, int nq, int k, int nprobe,
                                  const int32_t* d_q_filter, const int32_t* d_q_filter_mask, float* d_out_scores,
                                  int64_t* d_out_ids) {
    rass_engine* eng = v->eng;
    if (!flat || flat->eng != eng) return fail(RASS_ERR_INVALID, "the delta index must live on the IVF's engine");
    if (flat->dtype != RASS_F32 || flat->stride != v->stride || flat->dim != v->dim)
        return fail(RASS_ERR_UNSUPPORTED, "the delta index must be the fp32 index the IVF was built from");
    if (int rc = check_k(k)) return rc;
    if (d_q_filter_mask && !d_q_filter) return fail(RASS_ERR_INVALID, "q_filter_mask without q_filter");
    // the IVF's ids are ordinals of the source as it was laid out at build time (a loaded IVF trusts its first source)
    const int64_t epoch = flat->layout_epoch.load(std::memory_order_acquire);
    if (v->src_epoch < 0) v->src_epoch = epoch;
    if (v->src_epoch != epoch)
        return fail(RASS_ERR_INVALID, "the source index was compacted after this IVF was built (its ids are stale ordinals): rebuild the IVF");
    const int64_t rows = flat->rows.load(std::memory_order_acquire);
    const int64_t covered = v->src_rows;
    if (covered > rows) return fail(RASS_ERR_INVALID, "the IVF covers more rows than the delta index holds");
    const int64_t delta = rows - covered;
    if (delta > 0 && covered % 32 != 0)
        return fail(RASS_ERR_UNSUPPORTED, "an IVF with a delta must cover a multiple of 32 source rows (rass_ivf_build_prefix)");
    const bool gid = flat->has_gid.load(std::memory_order_acquire);
    hipStream_t st = eng->stream;
    float* ps = v->d_pair_scores;
    int64_t* pi = v->d_pair_ids;
    int rc = ivf_search_locked(v, d_queries, nq, k, nprobe, d_q_filter, d_q_filter_mask, ps, pi);
    if (rc != RASS_OK) return rc;
    int n_lists = 1;
    if (delta > 0) {
        const bool need_tags = (flat->deleted.load(std::memory_order_acquire) > 0) || (d_q_filter != nullptr);
        ScanRequest s = scan_request(eng);
        s.corpus = flat->d_rows + covered * flat->stride, s.n_rows = delta, s.stride = flat->stride;
        s.row_tag = need_tags ? flat->d_tags + covered : nullptr;
        s.queries = d_queries, s.q_dim = flat->dim, s.q_stride = flat->dim, s.nq = nq, s.q_filter = d_q_filter;
        s.k = k, s.id_base = covered, s.out_scores = ps + (int64_t)nq * k, s.out_ids = pi + (int64_t)nq * k;
        s.timing = eng;
        s.ext.d_q_mask = d_q_filter_mask;
        rc = scan_launch(s);
        if (rc != RASS_OK) return rc;
        n_lists = 2;
    }
    HIP_TRY(rass::launch_merge_topk(ps, pi, n_lists, nq, k, d_out_scores, d_out_ids, st, gid ? flat->d_gid : nullptr));
    return RASS_OK;
}

int rass_ivf_search_delta_device(rass_ivf_t* v, rass_index_t* flat, const float* d_queries, int nq, int k, int nprobe,
                                 const int32_t* d_q_filter, const int32_t* d_q_filter_mask, float* d_out_scores,
                                 int64_t* d_out_ids) {
    if (!v || !flat || !d_queries || !d_out_scores || !d_out_ids) return fail(RASS_ERR_INVALID, "NULL argument");
    if (int rc = check_nq(nq)) return rc;
    int rc = set_device(v->eng);
    if (rc != RASS_OK) return rc;
    std::lock_guard<std::mutex> lk(v->eng->mu);
    return ivf_delta_group_locked(v, flat, d_queries, nq, k, nprobe, d_q_filter, d_q_filter_mask, d_out_scores, d_out_ids);
}

// The host round trip of rass_ivf_search and rass_ivf_search_delta (flat = nullptr: no delta) on host_groups: launch groups
// of <= 32 queries through a pinned slot, the engine lock held while enqueuing only.
struct IvfHostCall {   // the caller's HOST arrays of a whole call: any nq
    const float* queries;
    int nq, k;
    const int32_t *q_filter, *q_filter_mask;
    float* out_scores;
    int64_t* out_ids;
};
static int ivf_search_host(rass_ivf_t* v, rass_index_t* flat, const IvfHostCall& r, int nprobe, int64_t* scanned_rows) {
    rass_engine* eng = v->eng;
    const int k = r.k;
    int64_t scanned_total = 0;
    const int rc = host_groups(
        eng, v->dim, r.queries, r.nq, r.q_filter, r.q_filter_mask, /*io_bytes=*/0, no_fill,
        [&](HostSlot* sl, int, int b) -> int {
            const int32_t* d_filter = r.q_filter ? eng->d_qfilter : nullptr;
            const int32_t* d_mask = r.q_filter_mask ? eng->d_qmask : nullptr;
            const int grc = flat ? ivf_delta_group_locked(v, flat, eng->d_qraw, b, k, nprobe, d_filter, d_mask, eng->d_out_scores, eng->d_out_ids)
                                 : ivf_search_locked(v, eng->d_qraw, b, k, nprobe, d_filter, d_mask, eng->d_out_scores, eng->d_out_ids);
            return grc != RASS_OK ? grc : slot_download(eng, sl, b, k, v->d_scanned);
        },
        [&](HostSlot* sl, int done, int b) -> int {
            memcpy(r.out_scores + (int64_t)done * k, sl->h_out_s, (size_t)b * k * 4);
            memcpy(r.out_ids + (int64_t)done * k, sl->h_out_i, (size_t)b * k * 8);
            scanned_total += *sl->h_scanned;   // the probe's fine scan, and the whole delta
            if (flat) scanned_total += std::max<int64_t>(0, flat->rows.load() - v->src_rows);
            return RASS_OK;
        });
    if (rc != RASS_OK) return rc;
    if (scanned_rows) *scanned_rows = scanned_total;
    return RASS_OK;
}

int rass_ivf_search_delta(rass_ivf_t* v, rass_index_t* flat, const float* queries, int nq, int k, int nprobe,
                          const int32_t* q_filter, const int32_t* q_filter_mask, float* out_scores, int64_t* out_ids,
                          int64_t* scanned_rows) {
    if (!v || !flat || !out_scores || !out_ids) return fail(RASS_ERR_INVALID, "NULL argument");
    if (nq < 0 || (nq > 0 && !queries)) return fail(RASS_ERR_INVALID, "bad queries / nq");
    if (int rc = check_k(k)) return rc;
    if (q_filter_mask && !q_filter) return fail(RASS_ERR_INVALID, "q_filter_mask without q_filter");
    return ivf_search_host(v, flat, {queries, nq, k, q_filter, q_filter_mask, out_scores, out_ids}, nprobe, scanned_rows);
}

// The block of rass_ivf_search_device_batch (rass_ivf::d_batch) for G groups.
struct IvfBatchView {
    float* q_all;            // [G][32][stride] normalised queries
    unsigned short* qb_all;  // bf16 / int8 slabs: the converted queries
    float* cs;               // coarse lists, cper elements per group
    int64_t* ci;
    float* fs;               // fine lists, fper elements per group
    int64_t* fi;
    int32_t *wt, *wr;        // work lists, `cap` items per group
    uint32_t* wm;
    int32_t* nw;             // [G] items per group
    int64_t* sc;             // [G] rows scanned per group
    float* cds;              // int8: the merged candidates [G][32][32]
    int64_t* cdr;
    size_t total;
};

static IvfBatchView ivf_batch_layout(unsigned char* base, const rass_ivf* v, int G, int64_t cper, int64_t fper) {
    Carver c{base};
    IvfBatchView L;
    const bool i8 = v->dtype == RASS_I8;
    const size_t cap = (size_t)v->total_tiles;
    L.q_all = c.take<float>((size_t)G * 32 * v->stride * 4);
    L.qb_all = c.take<unsigned short>(v->dtype != RASS_F32 ? (size_t)G * 32 * kMaxStride * 2 : 0);
    L.cs = c.take<float>((size_t)G * cper * 4);
    L.ci = c.take<int64_t>((size_t)G * cper * 8);
    L.fs = c.take<float>((size_t)G * fper * 4);
    L.fi = c.take<int64_t>((size_t)G * fper * 8);
    L.wt = c.take<int32_t>(G * cap * 4);
    L.wr = c.take<int32_t>(G * cap * 4);
    L.wm = c.take<uint32_t>(G * cap * 4);
    L.nw = c.take<int32_t>((size_t)G * 4);
    L.sc = c.take<int64_t>((size_t)G * 8);
    L.cds = c.take<float>(i8 ? (size_t)G * 32 * RASS_MAX_K * 4 : 0);
    L.cdr = c.take<int64_t>(i8 ? (size_t)G * 32 * RASS_MAX_K * 8 : 0);
    L.total = c.off;
    return L;
}

// Coarse workgroups per launch group of the batched probe: each leaves a top-np list per query, and the plan kernel merges a
// query's wpg * np <= 256 candidates.
static int ivf_batch_wpg(int nlist, int np) {
    const int n_ctiles = (nlist + 31) / 32;
    return std::max(1, std::min(8, std::min(n_ctiles, 256 / np)));
}

// A whole batch of launch groups (nq <= 1 024 queries) of an IVF probe with 4 + G launches instead of 5 G: ONE normalise,
// ONE grouped coarse scan (kFlatGroups: every group's 32 queries over the centroid slab, 8 workgroups per group), ONE plan
// launch (a workgroup per group; the coarse lists are merged inside it), the G fine scans over their groups' work lists,
// ONE grouped merge.  Same lists probed, same scores, same (score desc, id asc) order as rass_ivf_search_device group by
// group (tests/test_gpu_ivf.py).  nprobe <= 32 (deeper probes go group by group through the threshold path).
static int ivf_search_batch_locked(rass_ivf_t* v, const float* d_queries, int nq, int k, int nprobe,
                                   const int32_t* d_q_filter, float* d_out_scores, int64_t* d_out_ids,
                                   int64_t* d_scanned_per_group) {
    rass_engine* eng = v->eng;
    hipStream_t st = eng->stream;
    const int np = std::min(nprobe, v->nlist);
    const int G = (nq + RASS_MAX_QBATCH - 1) / RASS_MAX_QBATCH;
    const int wpg = ivf_batch_wpg(v->nlist, np);                                   // coarse workgroups per group
    const int64_t stride = v->stride;
    // fine-scan workgroups per group.  fp32 slab: ALL groups' fine scans are one launch (kIvfGroups) — the more groups, the
    // fewer workgroups each (32 at 32 groups: 1 024 in all, dispatched in group order, no launch boundary between groups);
    // bf16 slab: one launch per group over the whole chip.
    const bool one_fine_launch = v->dtype == RASS_F32 && ivf_batch_one_launch();
    const bool i8 = v->dtype == RASS_I8;
    if (i8 && k > kPrefilterMaxK) return fail(RASS_ERR_UNSUPPORTED, kIvfI8MaxKMsg);
    const int kf = i8 ? RASS_MAX_K : k;   // entries per fine list: the int8 scan keeps 32 candidates whatever k is
    int fgrid = scan_grid(v->total_tiles, kf, eng->n_cus);
    if (one_fine_launch) fgrid = std::max(1, std::min(fgrid, std::max(32, 1024 / G)));   // (both clamps are minima: their order does not matter)
    const int64_t cper = (int64_t)wpg * 32 * np;                                   // coarse list elements per group
    const int64_t fper = (int64_t)fgrid * 32 * kf;                                 // fine list elements per group
    const int64_t cap = v->total_tiles;
    int rc = grow_block(&v->d_batch, &v->batch_bytes, ivf_batch_layout(nullptr, v, G, cper, fper).total, st);
    if (rc != RASS_OK) return rc;
    const IvfBatchView L = ivf_batch_layout(v->d_batch, v, G, cper, fper);

    // (1) every query normalised and zero-padded, the groups' 32-row blocks back to back
    HIP_TRY(rass::launch_normalize_rows_f32(d_queries, v->dim, L.q_all, stride, nq, v->dim, st, (int64_t)G * 32));
    // (2) coarse: all groups in one launch
    {
        rass::ScanArgs a = ivf_centroid_args(v, L.q_all, L.cs, L.ci, 32, np);
        a.wgs_per_group = wpg;
        a.q_group_stride = 32 * stride;
        a.part_group_stride = cper;
        HIP_TRY(rass::launch_scan_topk_f32(a, G * wpg, st));
    }
    // (3) plan: one workgroup per group, the coarse lists merged inside
    HIP_TRY(rass::launch_plan_probe_groups(L.cs, L.ci, wpg, np, G, nq, cper, v->nlist, v->d_list_tile0, v->d_list_len, L.wt, L.wr,
                                           L.wm, cap, L.nw, L.sc, st, v->tile_rows));
    // (4) the fine scans, one per group, over the group's work list
    const int32_t* row_tag = (v->any_tags || d_q_filter != nullptr) ? v->d_tags : nullptr;
    if (v->dtype == RASS_BF16) HIP_TRY(rass::launch_queries_to_bf16(L.q_all, L.qb_all, (int64_t)G * 32 * stride, st));
    if (i8) HIP_TRY(rass::launch_queries_to_i8(L.q_all, L.qb_all, G * 32, stride, v->stride_i8, st));
    const int64_t q_low_bytes = i8 ? v->stride_i8 : stride * 2;   // bytes of one converted query
    auto group = [&](int g, int b) {   // group g with b queries (a batch takes no filter mask)
        return IvfGroup{L.q_all + (int64_t)g * 32 * stride, reinterpret_cast<const unsigned char*>(L.qb_all) + (int64_t)g * 32 * q_low_bytes,
                        d_q_filter ? d_q_filter + g * 32 : nullptr, nullptr, L.fs + g * fper, L.fi + g * fper, b};
    };
    if (one_fine_launch) {   // group 0 with the grouped fields added: all groups
        rass::ScanArgs a = ivf_f32_args(v, row_tag, group(0, 32), k);
        set_plan(a, IvfPlan{L.wt, L.wr, L.wm, L.nw, cap});
        a.wgs_per_group = fgrid;
        a.q_group_stride = 32 * stride;
        a.part_group_stride = fper;
        a.work_group_stride = cap;
        a.nq_total = nq;
        rc = timed_launch(eng, st, [&] { return HIP_RC(rass::launch_scan_topk_f32(a, G * fgrid, st)); });
        if (rc != RASS_OK) return rc;
    }
    for (int g = 0; g < G && !one_fine_launch; ++g) {
        const IvfPlan plan{L.wt + g * cap, L.wr + g * cap, L.wm + g * cap, L.nw + g, cap};
        rc = ivf_fine_scan(v, row_tag, group(g, std::min(RASS_MAX_QBATCH, nq - g * 32)), kf, plan, fgrid);
        if (rc != RASS_OK) return rc;
    }
    // (5) one grouped merge: slab positions -> source row ids (int8: the candidates of every group, then ONE exact re-rank)
    const rass::MergeGroups mg = dense_groups(nq, fper, (int64_t)RASS_MAX_QBATCH * kf, (int64_t)RASS_MAX_QBATCH * kf);
    rc = ivf_fine_merge(v, L.fs, L.fi, fgrid, nq, k, L.q_all, L.cds, L.cdr, &mg, d_out_scores, d_out_ids);
    if (rc != RASS_OK) return rc;
    if (d_scanned_per_group) HIP_TRY(hipMemcpyAsync(d_scanned_per_group, L.sc, (size_t)G * 8, hipMemcpyDeviceToDevice, st));
    return RASS_OK;
}

int rass_ivf_search_device_batch(rass_ivf_t* v, const float* d_queries, int nq, int k, int nprobe,
                                 const int32_t* d_q_filter, float* d_out_scores, int64_t* d_out_ids,
                                 int64_t* d_scanned_per_group) {
    if (!v || !d_queries || !d_out_scores || !d_out_ids) return fail(RASS_ERR_INVALID, "NULL argument");
    if (nq < 1 || nq > 32 * RASS_MAX_QBATCH) return fail(RASS_ERR_INVALID, "nq must be in [1, 1024]");
    if (int rc = check_k(k)) return rc;
    if (nprobe < 1) return fail(RASS_ERR_INVALID, "nprobe must be >= 1");
    int rc = set_device(v->eng);
    if (rc != RASS_OK) return rc;
    std::lock_guard<std::mutex> lk(v->eng->mu);
    const int np = std::min(nprobe, v->nlist);
    if (np > RASS_MAX_K || rass::plan_lds_bytes(v->nlist, ivf_batch_wpg(v->nlist, np), np) > rass::kPlanMaxLdsBytes) {
        // group by group: deep probes (the threshold path), and an IVF of so many lists that the batched plan's masks and
        // candidates do not fit one CU's LDS (nlist + 64 * wpg * np > 39 936: above 23 552 lists at nprobe 32).  Either way
        // the answer is rass_ivf_search_device's on each group of 32.
        for (int g = 0; g * RASS_MAX_QBATCH < nq; ++g) {
            const int b = std::min(RASS_MAX_QBATCH, nq - g * RASS_MAX_QBATCH);
            rc = ivf_search_locked(v, d_queries + (int64_t)g * RASS_MAX_QBATCH * v->dim, b, k, nprobe,
                                   d_q_filter ? d_q_filter + g * RASS_MAX_QBATCH : nullptr, nullptr,
                                   d_out_scores + (int64_t)g * RASS_MAX_QBATCH * k, d_out_ids + (int64_t)g * RASS_MAX_QBATCH * k);
            if (rc != RASS_OK) return rc;
            if (d_scanned_per_group)
                HIP_TRY(hipMemcpyAsync(d_scanned_per_group + g, v->d_scanned, 8, hipMemcpyDeviceToDevice, v->eng->stream));
        }
        return RASS_OK;
    }
    return ivf_search_batch_locked(v, d_queries, nq, k, nprobe, d_q_filter, d_out_scores, d_out_ids, d_scanned_per_group);
}

int rass_ivf_search_device(rass_ivf_t* v, const float* d_queries, int nq, int k, int nprobe,
                           const int32_t* d_q_filter, float* d_out_scores, int64_t* d_out_ids) {
    if (!v) return fail(RASS_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(v->eng->mu);
    return ivf_search_locked(v, d_queries, nq, k, nprobe, d_q_filter, nullptr, d_out_scores, d_out_ids);
}

int rass_ivf_search(rass_ivf_t* v, const float* queries, int nq, int k, int nprobe, const int32_t* q_filter,
                    float* out_scores, int64_t* out_ids, int64_t* scanned_rows) {
    if (!v || !out_scores || !out_ids) return fail(RASS_ERR_INVALID, "NULL argument");
    if (nq < 0 || (nq > 0 && !queries)) return fail(RASS_ERR_INVALID, "bad queries / nq");
    if (int rc = check_k(k)) return rc;
    return ivf_search_host(v, nullptr, {queries, nq, k, q_filter, nullptr, out_scores, out_ids}, nprobe, scanned_rows);
}

// ---- builds whose list plan runs on the GPU (ivf_build.hip): from a device-resident assignment, and an existing IVF
// extended over the rows its source took since, without retraining.  Both produce the IVF rass_ivf_build_prefix would produce
// from the same centroids and the same assignment, array by array (tests/test_gpu_ivf_absorb.py compares the saved files).
// Host traffic: total_tiles / live rows / status (24 bytes, sizes the slab), pos_of once (rass_ivf_delete reads it on the
// host), and the centroids of rass_ivf_build_device.

// The temporaries of a device-planned build; what is still set when it goes out of scope is released.
struct IvfPlanBlocks {
    int32_t *len = nullptr, *tile0 = nullptr, *pos = nullptr, *assign = nullptr;
    int64_t* ids = nullptr;
    int64_t* head = nullptr;   // [0] total_tiles, [1] live rows, [2] status (its low int32)
    void* ws = nullptr;
    ~IvfPlanBlocks() {
        for (void* p : {(void*)len, (void*)tile0, (void*)pos, (void*)assign, (void*)ids, (void*)head, ws})
            if (p) (void)hipFree(p);
    }
};

// The caller holds src->mu, has set the device and checked src / nlist / slab_dtype.  d_assign[n] on the device; centroids as
// ivf_build_tail takes them.  The plan's count phase sizes the slab, its place phase fills the slab's ids.
static int ivf_build_planned(rass_index* src, int nlist, const int32_t* d_assign, rass_dtype slab_dtype, int64_t n,
                             const float* centroids, const float* d_centroids_tile16, IvfPlanBlocks& t, rass_ivf_t** out) {
    hipStream_t st = src->eng->stream;
    const int tile_rows = slab_dtype == RASS_F32 ? 32 : 64;
    HIP_TRY(hipMalloc((void**)&t.len, (size_t)nlist * 4));
    HIP_TRY(hipMalloc((void**)&t.tile0, (size_t)nlist * 4));
    HIP_TRY(hipMalloc((void**)&t.pos, (size_t)std::max<int64_t>(n, 1) * 4));
    HIP_TRY(hipMalloc((void**)&t.head, 24));
    HIP_TRY(hipMalloc(&t.ws, rass::ivf_plan_workspace_bytes(n, nlist)));
    int32_t* d_status = reinterpret_cast<int32_t*>(t.head + 2);
    HIP_TRY(rass::launch_ivf_plan_count(d_assign, src->d_tags, n, nlist, tile_rows, t.len, t.tile0, t.head, t.head + 1, d_status,
                                        t.ws, st));
    int64_t head[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(head, t.head, 24, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t tiles = head[0];
    const int32_t status = (int32_t)(head[2] & 0xffffffffLL);
    if (status & 1) return fail(RASS_ERR_INVALID, "assign[] holds a list id outside [0, nlist)");
    if ((status & 2) || tiles * tile_rows > kMaxScanRows) return fail(RASS_ERR_UNSUPPORTED, "slab too large for one IVF shard");
    const int64_t slab_rows = std::max<int64_t>(tiles, 1) * tile_rows;
    HIP_TRY(hipMalloc((void**)&t.ids, (size_t)slab_rows * 8));
    HIP_TRY(rass::launch_ivf_plan_place(d_assign, src->d_tags, n, nlist, tile_rows, t.tile0, t.head, t.ids, slab_rows, t.pos, d_status,
                                        t.ws, st));
    // the count phase sized the slab: a place phase that disagrees with it must not be served
    int32_t status_after = 0;
    HIP_TRY(hipMemcpyAsync(&status_after, d_status, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (status_after != 0)
        return fail(RASS_ERR_HIP, "ivf build: the list plan's two phases disagree (the assignment or the tags changed under it)");
    const IvfListPlan plan{tiles, head[1], t.len, t.tile0, t.ids, t.pos, /*on_device=*/true};
    return ivf_build_tail(src, nlist, slab_dtype, n, plan, centroids, d_centroids_tile16, out);
}

int rass_ivf_build_device(rass_index_t* src, const float* centroids, int nlist, const int32_t* d_assign, rass_dtype slab_dtype,
                          int64_t n_rows, rass_ivf_t** out) {
    if (!src || !centroids || !d_assign || !out) return fail(RASS_ERR_INVALID, "NULL argument");
    *out = nullptr;
    int rc = ivf_source_check(src, nlist, slab_dtype);
    if (rc != RASS_OK) return rc;
    std::lock_guard<std::mutex> lk(src->mu);
    rc = set_device(src->eng);
    if (rc != RASS_OK) return rc;
    if (n_rows > src->rows) return fail(RASS_ERR_INVALID, "n_rows exceeds the rows of the source index");
    const int64_t n = n_rows < 0 ? src->rows.load() : n_rows;
    IvfPlanBlocks t;
    return ivf_build_planned(src, nlist, d_assign, slab_dtype, n, centroids, nullptr, t, out);
}

int rass_ivf_absorb(rass_ivf_t* ivf, rass_index_t* src, int64_t n_rows, rass_ivf_t** out) {
    if (!ivf || !src || !out) return fail(RASS_ERR_INVALID, "NULL argument");
    *out = nullptr;
    rass_engine* eng = src->eng;
    const rass_dtype slab_dtype = (rass_dtype)ivf->dtype;
    int rc = ivf_source_check(src, ivf->nlist, slab_dtype);
    if (rc != RASS_OK) return rc;
    if (ivf->eng != eng) return fail(RASS_ERR_INVALID, "the source index must live on the IVF's engine");
    if (src->stride != ivf->stride || src->dim != ivf->dim)
        return fail(RASS_ERR_INVALID, "the source index is not the one the IVF was built from (dim)");
    std::lock_guard<std::mutex> lk(src->mu);
    rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    // the IVF's ids are ordinals of the source as it was laid out at build time (a loaded IVF trusts its source, as the search does)
    if (ivf->src_epoch >= 0 && ivf->src_epoch != src->layout_epoch.load(std::memory_order_acquire))
        return fail(RASS_ERR_INVALID, "the source index was compacted after this IVF was built (its ids are stale ordinals): rebuild the IVF");
    const int64_t rows = src->rows.load(), covered = ivf->src_rows;
    if (n_rows > rows) return fail(RASS_ERR_INVALID, "n_rows exceeds the rows of the source index");
    const int64_t n = n_rows < 0 ? rows : n_rows;
    if (n < covered) return fail(RASS_ERR_INVALID, "n_rows is below the rows the IVF already covers (rass_ivf_covered_rows)");
    if (n % 32 != 0 && n != rows)
        return fail(RASS_ERR_INVALID, "n_rows must be a multiple of 32 or every row of the source (the delta must start on a scan tile)");
    hipStream_t st = eng->stream;
    IvfPlanBlocks t;
    const int64_t n_padded = std::max<int64_t>((n + 31) / 32 * 32, 32);
    HIP_TRY(hipMalloc((void**)&t.assign, (size_t)n_padded * 4));
    // rows the old slab does not hold are tombstones of the source: their entries are never read as a list
    HIP_TRY(hipMemsetAsync(t.assign, 0, (size_t)n_padded * 4, st));
    // new rows: their nearest centroid, whole 32-row blocks from the one the covered rows end in (ties -> lowest list, as a build) ...
    const int64_t first_block = covered / 32, n_blocks = (n + 31) / 32 - first_block;
    if (n > covered) {
        rass::AssignArgs a;
        a.rows = src->d_rows;
        a.centroids = ivf->d_centroids;
        a.assign = t.assign + first_block * 32;
        a.best = nullptr;
        a.row_stride = src->stride;
        a.slab_rows = src->capacity;
        a.first_block = first_block;
        a.block_step = 1;
        a.n_blocks = (int)n_blocks;
        a.nlist = ivf->nlist;
        HIP_TRY(rass::launch_kmeans_assign_f32(a, eng->n_cus, st));
    }
    // ... covered rows keep their list (written second: the covered rows of a shared block win)
    HIP_TRY(rass::launch_ivf_lists_to_assign(ivf->d_list_tile0, ivf->d_list_len, ivf->nlist, ivf->tile_rows, ivf->d_ids,
                                             ivf->slab_rows, t.assign, covered, st));
    return ivf_build_planned(src, ivf->nlist, t.assign, slab_dtype, n, nullptr, ivf->d_centroids, t, out);
}

int rass_ivf_lists_device(rass_ivf_t* ivf, int32_t* d_assign, int64_t assign_capacity, int32_t* d_list_len) {
    if (!ivf) return fail(RASS_ERR_INVALID, "NULL argument");
    if (d_assign && assign_capacity < ivf->src_rows)
        return fail(RASS_ERR_INVALID, "assign_capacity is smaller than the rows the IVF covers (rass_ivf_covered_rows)");
    rass_engine* eng = ivf->eng;
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    std::lock_guard<std::mutex> lk(eng->mu);
    hipStream_t st = eng->stream;
    if (d_assign && ivf->src_rows > 0) {
        HIP_TRY(hipMemsetAsync(d_assign, 0xff, (size_t)ivf->src_rows * 4, st));
        HIP_TRY(rass::launch_ivf_lists_to_assign(ivf->d_list_tile0, ivf->d_list_len, ivf->nlist, ivf->tile_rows, ivf->d_ids,
                                                 ivf->slab_rows, d_assign, ivf->src_rows, st));
    }
    if (d_list_len) HIP_TRY(hipMemcpyAsync(d_list_len, ivf->d_list_len, (size_t)ivf->nlist * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RASS_OK;
}

size_t rass_ivf_plan_workspace_bytes(int64_t n_rows, int nlist) {
    return (n_rows < 0 || nlist < 1 || nlist > kIvfMaxLists) ? 0 : rass::ivf_plan_workspace_bytes(n_rows, nlist);
}

int rass_ivf_plan_lists(const int32_t* d_assign, const int32_t* d_tags, int64_t n_rows, int nlist, int tile_rows,
                        int32_t* d_list_len, int32_t* d_list_tile0, int64_t* d_total_tiles, int64_t* d_slab_ids,
                        int64_t slab_ids_capacity, int32_t* d_pos_of, int32_t* d_status, void* d_workspace, size_t workspace_bytes,
                        void* stream) {
    if (n_rows < 0 || n_rows > kMaxScanRows) return fail(RASS_ERR_INVALID, "n_rows must be in [0, 0x7fffffc0]");
    if (nlist < 1 || nlist > kIvfMaxLists) return fail(RASS_ERR_INVALID, "nlist must be in [1, 32768]");
    if (tile_rows != 32 && tile_rows != 64) return fail(RASS_ERR_INVALID, "tile_rows must be 32 or 64");
    if (slab_ids_capacity < tile_rows || slab_ids_capacity > kMaxScanRows)
        return fail(RASS_ERR_INVALID, "slab_ids_capacity must hold at least one tile and at most 0x7fffffc0 rows");
    if (!d_list_len || !d_list_tile0 || !d_total_tiles || !d_slab_ids || !d_status || !d_workspace)
        return fail(RASS_ERR_INVALID, "NULL argument");
    if (n_rows > 0 && (!d_assign || !d_tags || !d_pos_of)) return fail(RASS_ERR_INVALID, "NULL argument");
    if (workspace_bytes < rass::ivf_plan_workspace_bytes(n_rows, nlist))
        return fail(RASS_ERR_INVALID, "workspace too small (rass_ivf_plan_workspace_bytes)");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(rass::launch_ivf_plan_count(d_assign, d_tags, n_rows, nlist, tile_rows, d_list_len, d_list_tile0, d_total_tiles, nullptr,
                                        d_status, d_workspace, st));
    HIP_TRY(rass::launch_ivf_plan_place(d_assign, d_tags, n_rows, nlist, tile_rows, d_list_tile0, d_total_tiles, d_slab_ids,
                                        slab_ids_capacity, d_pos_of, d_status, d_workspace, st));
    return RASS_OK;
}

}  // extern "C"
