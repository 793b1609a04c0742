// gemm_route.cpp — the routing rule of the encoder GEMMs (gemm_route.h).  Plain C++: no device, no HIP.
#include "gemm_route.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace rass {

namespace {
constexpr int GBM = 128, GBN = 128, GBK = 64;   // tile of the 128^2 family (gemm_common.h)
constexpr int RBM = 256, RBN = 256;             // tile of the persistent kernels

GemmSwitches read_switches() {
    GemmSwitches sw;
    const char* v = rass_env("RASS_GEMM_FEWROWS");
    sw.fewrows = !(v && v[0] == '0');
    v = rass_env("RASS_GEMM_FEWROWS_MAX");
    const int m = v ? atoi(v) : 96;   // 128 until the end of round 4: from 97 rows the four-stage kernel (mid_enabled) is faster
    sw.fewrows_max_rows = m < 16 ? 16 : (m > 128 ? 128 : m);
    v = rass_env("RASS_GEMM_FEWROWS_RES");
    sw.fewrows_residual_max_rows = v ? atoi(v) : 64;   // 32 until the end of round 4 (see route_gemm_residual_layernorm)
    v = rass_env("RASS_GEMM_MID");   // 0: round 3's paths (two-buffer kernel / split-K pair); 2: every shape (the A/Bs)
    sw.mid = v != nullptr && atoi(v) == 0 ? 0 : v != nullptr && atoi(v) == 2 ? 2 : -1;
    v = rass_env("RASS_GEMM_VARIANT");
    sw.variant = v != nullptr && strcmp(v, "p5") == 0 ? 5 : v != nullptr && strcmp(v, "p4") == 0 ? 4 : 0;
    v = rass_env("RASS_GEMM_SPLITK_S");   // sweeps (scripts/probe_gemm_mid.py)
    sw.splitk_s = v ? atoi(v) : -1;
    if (v && sw.splitk_s < 0) sw.splitk_s = 0;
    v = rass_env("RASS_GEMM_MID_BM");
    sw.mid_bm = v ? (atoi(v) == 128 ? 128 : 64) : 0;
    v = rass_env("RASS_GEMM_GRID");   // experiment: fewer persistent workgroups than CUs (per-CU vs chip-wide limits)
    sw.grid = v && atoi(v) >= 1 ? atoi(v) : 0;
    v = rass_env("RASS_P5_POLICY");   // A/B: 0 = plain output stores
    sw.p5_policy = v && atoi(v) == 0 ? 0 : 1;
    v = rass_env("RASS_GEMM_LNIN_WAVES");   // 4: the 4-wave workgroups of rounds 2-3 (A/B)
    sw.lnin_waves = v && atoi(v) == 4 ? 4 : 16;
    v = rass_env("RASS_ENCODER_LN_FOLD");
    sw.ln_fold = !(v && atoi(v) == 0);
    return sw;
}
}  // namespace

const GemmSwitches& gemm_switches() {
    thread_local GemmSwitches sw;
    thread_local unsigned long scope = 0;   // (rass_env scopes start at 1)
    if (scope != rass_env_scope()) {
        sw = read_switches();
        scope = rass_env_scope();
    }
    return sw;
}

namespace {
// Where it pays (scripts/probe_encoder_shapes.py, whole forwards, same box): 129 .. 1 024 rows.  The K loop is not what bounds it —
// hand-scheduling it changed nothing: a workgroup keeps ~4 operand tiles (128 KiB) in flight against ~2 us of global -> LDS
// latency, i.e. ~60 GB/s per CU, and a 128 x 128 tile moves 512 KiB for K = 1 024 (15 us per GEMM on the 72-96 CUs such a
// batch occupies).  64-ROW tiles (while they still fit one per CU) put twice the CUs to work on 3/4 of the bytes each:
// 32 x 12 tokens 1.887 -> 1.51 ms per forward, 16 x 12: 1.610 -> 1.415; 64 x 12 (128-row tiles: 144 workgroups) 2.144 -> 1.99,
// 32 x 32: 2.228 -> 2.04.  Below 129 rows the split-K pair's workgroups win (8 x 12: 1.333 vs 1.376), from 1 536 rows on the
// two-buffer kernel's two workgroups per CU (48 x 32: 2.515 vs 2.59).
bool mid_enabled(const GemmSwitches& sw, int M) {
    if (sw.mid == 0) return false;
    if (sw.mid == 2) return true;
    return M > 96 && M <= 8 * GBM;   // (from 129 rows until the end of round 4; 97 .. 128 rows: 120 tokens 1.44 -> 1.31 ms per forward)
}

// with the four-stage kernel a short K (<= 16 steps) is not split any more: one launch with the epilogue fused beats the
// pair (see gemm_bf16_mid_kernel)
bool mid_takes_short_k(const GemmSwitches& sw, int M, int K) { return mid_enabled(sw, M) && K <= 1024 && K >= 4 * GBK; }

// the four-stage and p4 kernels address their operands through 32-bit buffer descriptors
bool operands_fit_descriptors(const GemmShape& s) {
    return (uint64_t)s.M_pad * s.K * 2 < (1ull << 32) - (1ull << 24) && (uint64_t)s.N * s.K * 2 < (1ull << 32) - (1ull << 24);
}

    // big shapes: the persistent 256^2 kernel (p5); everything else: the 128^2 kernel.  "Big" = enough 256^2 tiles to
    // keep most of the chip's CUs busy (a persistent kernel runs one tile per CU at a time): a 2 048-token upload has
    // 32 tiles at N = 1024 and ran on 32 of 256 CUs; as 128^2 tiles (split over K where those are few) it fills the
    // chip.  RASS_GEMM_VARIANT=p5 keeps the persistent kernel for every shape it accepts (A/B runs, tests).
bool persistent_shape(const GemmShape& s, bool any_tile_count) {
    return s.N % RBN == 0 && s.M_pad % RBM == 0 && s.K % 64 == 0 && s.K >= 128 && s.M >= 1024 &&
           (any_tile_count || (int64_t)(s.N / RBN) * (s.M_pad / RBM) >= 192);
}

// tokens <= 64; K = whole 256-deep trips per wave: 4 waves per workgroup (K <= 3072), 16 for whole multiples of 4096
// RASS_GEMM_FEWROWS_MAX=<rows> (A/B; read per launch): the one-launch kernel up to that many rows where its partial tiles fit
// (4 waves: K <= 3072); default 128 (r03: 96 tokens 1.405 -> 1.337 ms per forward, 128 tokens 1.539 -> 1.495)
int fewrows_waves(int M, int N, int K, const GemmSwitches& sw) {
    if (M < 1 || N % 16 != 0 || N < 1024) return 0;
    if (K % 1024 == 0 && K <= 3072) return M <= sw.fewrows_max_rows ? 4 : 0;
    if (M > 64) return 0;                        // 16 waves x 8 row blocks of partial tiles would not fit the static LDS
    if (K % 4096 == 0 && K <= 8192) return 16;
    return 0;
}

// Number of K slices for a GEMM with few output tiles (0 = do not split), whole 64-deep steps per slice, a scratch of
// S * M_pad * N floats that fits.  Measured on MI355X (scripts/probe_gemm_mid.py, profiles/r03_gemm_mid_sweep.txt; every
// combination of the four encoder GEMMs x 128 .. 3 072 rows x S): what bounds these kernels is the rate at which ONE CU
// can fill its LDS (one 128^2 workgroup takes ~0.9 us per 64-deep step however deep its prefetch ring is — a four-slot
// ring with counted waits measured the SAME times as this two-buffer loop and was removed), so a short K (1 024) wants
// >= 128 workgroups of >= 4 steps and a long K (4 096) up to 512 workgroups of >= 16 steps; beyond that the fp32 partials
// cost more than the split wins.  The rule was then settled on whole forwards (cold weights: scripts/sweep_splitk_rule.sh,
// same file), where more workgroups pull harder on HBM than the warm micro-benchmark shows.  Round 2 split only below 96
// tiles and aimed at 128 workgroups: FFN-down ran 64 serial steps at 96+ tiles (1 024 rows 29 -> 22 us, 1 536 rows
// 45 -> 28, 2 048 rows 46 -> 34).
int splitk_slices(int M_pad, int N, int K, size_t ws_bytes, const GemmSwitches& sw) {
    const int tiles = (N / GBN) * (M_pad / GBM), steps = K / GBK;
    if (sw.splitk_s >= 0) {
        const int S = sw.splitk_s;
        if (S < 2 || S > 16 || steps % S != 0 || (size_t)S * M_pad * N * sizeof(float) > ws_bytes) return 0;
        return S;
    }
    if (steps < 2) return 0;
    int S = 1;
    if (K < 2048) {
        // short K (16 steps): the smallest split that gives >= 128 workgroups, slices of >= 4 steps
        while (S < 4 && tiles * S < 128 && steps % (2 * S) == 0) S *= 2;
    } else {
        // long K (64 steps): the largest split that stays within 512 workgroups (two resident per CU); slices of >= 16 steps
        // from 48 tiles on, >= 8 below, >= 4 for a single row of tiles
        const int cap = tiles <= 8 ? 16 : tiles < 48 ? 8 : 4;
        while (S < cap && tiles * S * 2 <= 512 && steps % (2 * S) == 0) S *= 2;
    }
    while (S > 1 && (size_t)S * M_pad * N * sizeof(float) > ws_bytes) S /= 2;
    return S > 1 ? S : 0;
}

// The persistent GEMM of big shapes is p4 since round 4; RASS_GEMM_VARIANT=p5 brings back the 8-wave kernel (the A/B; same bits).
GemmRoute route_persistent(const GemmShape& s, int epilogue, const GemmSwitches& sw, int n_cus) {
    GemmRoute r;
    r.tiles = (s.N / RBN) * (s.M_pad / RBM);
    r.grid = r.tiles < n_cus ? r.tiles : n_cus;
    if (sw.grid >= 1 && sw.grid < r.grid) r.grid = sw.grid;
    // (the folded GELU epilogue, EPI 5, is the one p4 loses: 1 165 vs 1 129 us per FFN-up — a single wave per SIMD has nothing to
    // overlap that epilogue's dependency stalls with; it stays on p5 unless RASS_GEMM_VARIANT=p4 asks for p4 everywhere)
    const bool p4 = sw.variant == 5 ? false : sw.variant == 4 ? true : epilogue != 5;
    r.kind = p4 && s.K >= 512 && operands_fit_descriptors(s) ? GemmKind::P4 : GemmKind::P5;
    r.policy = r.kind == GemmKind::P5 ? sw.p5_policy : 1;
    return r;
}
}  // namespace

GemmRoute route_gemm(const GemmShape& s, int epilogue, bool has_ws, size_t ws_bytes, const GemmSwitches& sw, int n_cus) {
    const int M = s.M, M_pad = s.M_pad, N = s.N, K = s.K;
    GemmRoute r;
    // every kernel here works on whole 128-row / 128-column tiles and 64-deep K steps (include/rass_engine.h)
    if (M < 1 || M_pad < M || N <= 0 || K <= 0 || M_pad % GBM != 0 || N % GBN != 0 || K % GBK != 0 || epilogue < 0 || epilogue > 5)
        return r;
    if (epilogue >= 3)   // the LayerNorm fold: the persistent kernels, where the default rule puts a shape on them
        return persistent_shape(s, false) ? route_persistent(s, epilogue, sw, n_cus) : r;
    // a few rows against a wide matrix: one launch, epilogue included (query-time embedding; chosen with the scratch
    // lent, i.e. on the same calls that would otherwise be split over K)
    if (const int fw = has_ws && M_pad >= 64 && sw.fewrows ? fewrows_waves(M, N, K, sw) : 0) {
        r.kind = GemmKind::FewRows;
        r.waves = fw;
        r.row_blocks = (M + 15) / 16;
        return r;
    }
    // few rows: split K over more workgroups (the caller lends the fp32 scratch)
    if (has_ws && !mid_takes_short_k(sw, M, K)) {
        const int mp = (M + GBM - 1) / GBM * GBM;   // whole 128-row tiles that hold real rows (<= M_pad)
        if (const int S = splitk_slices(mp, N, K, ws_bytes, sw)) {
            r.kind = GemmKind::SplitK;
            r.slices = S;
            r.rows_pad = mp;
            return r;
        }
    }
    if (persistent_shape(s, sw.variant != 0)) return route_persistent(s, epilogue, sw, n_cus);
    if (mid_enabled(sw, M) && K >= 4 * GBK && operands_fit_descriptors(s)) {
        // 64-row tiles while 128-row ones would leave CUs idle (RASS_GEMM_MID_BM=128 / 64: the A/B)
        r.kind = GemmKind::Mid;
        r.bm = (N / GBN) * ((M + 63) / 64) <= 256 ? 64 : 128;   // 64-row tiles while they still fit one per CU
        if (sw.mid_bm != 0) r.bm = sw.mid_bm;
        r.grid = (N / GBN) * ((M + r.bm - 1) / r.bm);
        return r;
    }
    r.kind = GemmKind::Tile128;
    r.grid = (N / GBN) * (M_pad / GBM);
    return r;
}

// the residual GEMMs (N = hidden) take the one-launch kernel only for the fewest rows: from 3 row blocks on the split-K
// pair is faster (measured at 48 and 64 tokens); RASS_GEMM_FEWROWS_RES=<rows> moves the limit (A/B)
ResidualRoute route_gemm_residual_layernorm(const GemmShape& s, bool has_ws, size_t ws_bytes, const GemmSwitches& sw) {
    const int M = s.M, M_pad = s.M_pad, N = s.N, K = s.K;
    ResidualRoute r;
    // a query's few rows: the one-launch GEMM (bias + residual in its epilogue) and the row-wise LayerNorm — two launches
    // like the split-K pair below, but 5 + 5 us where that pair takes 6 + 7.4 (16 slices read back by 16 waves)
    // (a K of whole 4096s runs as four K slices of 4-wave workgroups: what must fit is a slice)
    if (has_ws && M_pad >= 64 && sw.fewrows && M <= sw.fewrows_residual_max_rows &&
        fewrows_waves(M, N, K % 4096 == 0 ? K / 4 : K, sw) != 0) {
        // K = 4096 (FFN-down): 64 workgroups of 16 waves took 9.4 us; 4 x 64 workgroups of 4 waves write partial tiles and
        // the fused reduce + residual + LayerNorm kernel (4 slices) follows
        const int rows_pad = M <= 64 ? 64 : 128;
        if (K % 4096 == 0 && K / 4 <= 3072 && N % 8 == 0 && N <= 2048 && (size_t)4 * rows_pad * N * sizeof(float) <= ws_bytes) {
            r.tail = ResidualTail::FewRows4Ln;
            r.slices = 4;
            r.rows_pad = rows_pad;
        }
        r.few_rows = true;
        return r;
    }
    if (has_ws && M_pad % GBM == 0 && N % GBN == 0 && K % GBK == 0 && N % 8 == 0 && N <= 2048 && !mid_takes_short_k(sw, M, K)) {
        const int mp = (M + GBM - 1) / GBM * GBM;
        if (const int S = splitk_slices(mp, N, K, ws_bytes, sw)) {
            r.tail = ResidualTail::SplitKLn;
            r.slices = S;
            r.rows_pad = mp;
        }
    }
    return r;
}

bool gemm_ln_input_shape_ok(int M, int N, int K, const GemmSwitches& sw) {
    return M >= 1 && M <= 32 && K == 1024 && N % 16 == 0 && N >= 1024 && sw.fewrows;
}

bool gemm_fold_ok(int M, int M_pad, int hidden, int intermediate, const GemmSwitches& sw) {
    return sw.ln_fold && hidden % 256 == 0 && persistent_shape({M, M_pad, hidden, hidden}, false) &&
           persistent_shape({M, M_pad, 3 * hidden, hidden}, false) && persistent_shape({M, M_pad, intermediate, hidden}, false) &&
           persistent_shape({M, M_pad, hidden, intermediate}, false);
}

namespace {
void gemm_label(const GemmRoute& r, char* out, size_t n) {
    switch (r.kind) {
        case GemmKind::FewRows: snprintf(out, n, "fewrows%d", r.waves); break;
        case GemmKind::SplitK: snprintf(out, n, "splitk%d", r.slices); break;
        case GemmKind::Mid: snprintf(out, n, "mid%d", r.bm); break;
        case GemmKind::Tile128: snprintf(out, n, "tile128"); break;
        case GemmKind::P4: snprintf(out, n, "p4"); break;
        case GemmKind::P5: snprintf(out, n, "p5"); break;
        default: snprintf(out, n, "unsupported"); break;
    }
}
}  // namespace

void gemm_route_label(int entry, const GemmShape& s, int epilogue, size_t ws_bytes, const GemmSwitches& sw, char* out, size_t n) {
    const bool has_ws = ws_bytes > 0;
    snprintf(out, n, "unsupported");
    if (entry == 0 && epilogue >= 0 && epilogue <= 2) {
        gemm_label(route_gemm(s, epilogue, has_ws, ws_bytes, sw, 256), out, n);
    } else if (entry == 1 && s.M >= 1 && s.M_pad >= s.M && s.N > 0 && s.K > 0) {
        const ResidualRoute r = route_gemm_residual_layernorm(s, has_ws, ws_bytes, sw);
        if (r.tail == ResidualTail::FewRows4Ln) {
            snprintf(out, n, "fewrows4+ln");
        } else if (r.tail == ResidualTail::SplitKLn) {
            snprintf(out, n, "splitk%d+ln", r.slices);
        } else {   // the GEMM on its own route, then the LayerNorm launch
            if (route_gemm(s, 1, has_ws, ws_bytes, sw, 256).kind != GemmKind::Unsupported) snprintf(out, n, r.few_rows ? "fewrows+pair" : "pair");
        }
    } else if (entry == 2 && (epilogue == 0 || epilogue == 2)) {
        if (gemm_ln_input_shape_ok(s.M, s.N, s.K, sw)) snprintf(out, n, "lnin%d", sw.lnin_waves);
    } else if (entry == 3 && epilogue >= 3 && epilogue <= 5) {
        gemm_label(route_gemm(s, epilogue, false, 0, sw, 256), out, n);
    }
}

}  // namespace rass
