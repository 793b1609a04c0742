// gemm_route.h — which kernel an encoder GEMM gets.  Host-only and pure: route_gemm() and route_gemm_residual_layernorm()
// are functions of the shape, the epilogue, the scratch lent and the switches; encoder_gemm.hip validates, routes, and
// switches on the kind.  DESIGN.md §4 has the table with the measurements behind every boundary.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace rass {

const char* rass_env(const char* name);   // encoder_kernels.h
unsigned long rass_env_scope();

// Every RASS_GEMM_* / RASS_P5_POLICY / RASS_ENCODER_LN_FOLD switch (A/B and diagnostic), parsed.
struct GemmSwitches {
    bool fewrows = true;                  // RASS_GEMM_FEWROWS=0: the split-K pair instead of the one-launch few-rows kernels
    int fewrows_max_rows = 96;            // RASS_GEMM_FEWROWS_MAX, 16 .. 128
    int fewrows_residual_max_rows = 64;   // RASS_GEMM_FEWROWS_RES
    int mid = -1;                         // RASS_GEMM_MID: 0 never, 2 every shape, -1 (default) 97 .. 1 024 rows
    int variant = 0;                      // RASS_GEMM_VARIANT: 4 = p4, 5 = p5 for every shape the persistent kernels accept; 0 default
    int splitk_s = -1;                    // RASS_GEMM_SPLITK_S: that many slices or no split; -1 unset
    int mid_bm = 0;                       // RASS_GEMM_MID_BM: 128 / 64; 0 unset
    int grid = 0;                         // RASS_GEMM_GRID: fewer persistent workgroups than CUs; 0 unset
    int p5_policy = 1;                    // RASS_P5_POLICY=0: plain output stores
    int lnin_waves = 16;                  // RASS_GEMM_LNIN_WAVES=4: the 4-wave LN-input workgroups
    bool ln_fold = true;                  // RASS_ENCODER_LN_FOLD=0: no LayerNorm fold
};
// The switches of the current rass_env scope (read once per scope and thread): the only reader of these names in the library.
const GemmSwitches& gemm_switches();

enum class GemmKind { Unsupported, FewRows, SplitK, Mid, Tile128, P4, P5 };

struct GemmShape {
    int M, M_pad, N, K;
};

struct GemmRoute {
    GemmKind kind = GemmKind::Unsupported;
    int waves = 0;        // FewRows: 4 or 16 waves per workgroup
    int row_blocks = 0;   // FewRows: 16-row blocks
    int slices = 0;       // SplitK: K slices
    int rows_pad = 0;     // SplitK: the whole 128-row tiles that hold real rows
    int bm = 0;           // Mid: rows per tile, 64 or 128
    int grid = 0;         // Mid / Tile128: tiles; P4 / P5: persistent workgroups
    int tiles = 0;        // P4 / P5: 256 x 256 tiles
    int policy = 1;       // P5: store policy (POL)
};

// launch_gemm_bf16 (epilogue 0 / 1 / 2) and launch_gemm_bf16_fold (3 / 4 / 5: persistent kernels only)
GemmRoute route_gemm(const GemmShape& s, int epilogue, bool has_ws, size_t ws_bytes, const GemmSwitches& sw, int n_cus);

// launch_gemm_bf16_residual_layernorm: how the sum is reduced and normalised
enum class ResidualTail {
    FewRows4Ln,   // four K slices of 4-wave few-rows workgroups, then the fused reduce + residual + LayerNorm
    SplitKLn,     // split-K partial tiles, then the fused reduce + residual + LayerNorm
    GemmThenLn,   // launch_gemm_bf16 (epilogue 1, routed by route_gemm) into `y`, then launch_layernorm
};
struct ResidualRoute {
    ResidualTail tail = ResidualTail::GemmThenLn;
    int slices = 0;      // FewRows4Ln: 4; SplitKLn: S
    int rows_pad = 0;    // rows of a partial tile
    bool few_rows = false;   // chosen under the residual few-rows rule (<= fewrows_residual_max_rows rows): label fewrows+pair
};
ResidualRoute route_gemm_residual_layernorm(const GemmShape& s, bool has_ws, size_t ws_bytes, const GemmSwitches& sw);

bool gemm_ln_input_shape_ok(int M, int N, int K, const GemmSwitches& sw);                    // launch_gemm_bf16_ln_input
bool gemm_fold_ok(int M, int M_pad, int hidden, int intermediate, const GemmSwitches& sw);   // all four GEMMs of a layer

// The route as a short label (rass_gemm_bf16_route): entry 0 gemm_ws, 1 residual_layernorm, 2 ln_input, 3 fold.
void gemm_route_label(int entry, const GemmShape& s, int epilogue, size_t ws_bytes, const GemmSwitches& sw, char* out, size_t out_bytes);

}  // namespace rass
