// Launch planning of the convolution template, for nc_conv.hip alone (nc_conv.h is included by every instantiation unit): the list of
// instance families with the one lookup over it, and the plan launch_conv makes before it launches.
#pragma once
#include "nc_conv.h"

namespace nc {

typedef void (*conv_kernel_fn)(const ConvArgs);

// ---- the instances of the template ------------------------------------------------------------------------------------------
// Every instantiation unit (nc_conv_k*.hip, nc_conv_in2*.hip, nc_conv_xv*.hip) exports one table function per family it holds.  This
// list is the only place that names them: an instance family is added here and in its unit.
// Plain instances: conv_kernel_table_k<K>(TM, TN), with the reduction block CB and the staging depth NX they were compiled for.
#define NC_K_CASES(X) X(1) X(2) X(3) X(4) X(6) X(7) X(8) X(10) X(16)
// The other families: X(form, taps, table function suffix, table arguments, CB, NX); CB = 0: CB and NX of the plain instance of the taps.
#define NC_CONV_FAMILIES(X)                                                                                                          \
    X(FUSED, 7, fused_k7, TMTN, 0, 0)        X(FUSEDW, 7, fusedw_k7, TMTN, 4, 5)                                                      \
    X(XV, 7, xv_k7, TM, 0, 0)                X(XV_FUSED, 7, xv_fused_k7, TM, 0, 0)                                                    \
    X(XV_SUB, 2, xv_sub_k2, TM, 0, 0)        X(XV_SUBG, 2, xv_subg_k2, TM, 0, 0)                                                      \
    X(DIST, 16, dist_k16, TMTN, 0, 0)        X(DIST_SUB, 2, dist_sub_k2, TMTN, 0, 0)                                                  \
    X(IN2, 2, in2_k2, TMTN, 0, 0)            X(IN2, 4, in2_k4, TMTN, 0, 0)            X(IN2, 8, in2_k8, TMTN, 0, 0)                   \
    X(IN2, 10, in2_k10, TMTN, 0, 0)          X(IN2, 16, in2_k16, TMTN, 0, 0)          X(IN2_SUB, 2, in2_sub_k2, TMTN, 0, 0)           \
    X(SUB, 2, sub_k2, TMTN, 0, 0)            X(SUB_NARROW, 2, sub_narrow_k2, TM, 0, 0) X(SUBG, 2, subg_k2, TMTN, 0, 0)                \
    X(NARROW, 2, narrow_k2, TM, 0, 0)        X(NARROW, 3, narrow_k3, TM, 0, 0)        X(NARROW, 7, narrow_k7, TM, 0, 0)               \
    X(NARROW, 16, narrow_k16, TM, 0, 0)      X(SLIM, 3, slim_k3, TMTN, 8, 10)         X(SLIM, 7, slim_k7, TMTN, 4, 5)
#define NC_TABLE_DECL_TMTN int, int
#define NC_TABLE_DECL_TM int
#define NC_TABLE_CALL_TMTN TM, TN
#define NC_TABLE_CALL_TM TM

#define X(k) conv_kernel_fn conv_kernel_table_k##k(int, int); int conv_kernel_cb_k##k(); int conv_kernel_nx_k##k();
NC_K_CASES(X)
#undef X
#define X(form, k, name, args, cb, nx) conv_kernel_fn conv_kernel_table_##name(NC_TABLE_DECL_##args);
NC_CONV_FAMILIES(X)
#undef X

enum ConvForm { F_PLAIN, F_NARROW, F_SLIM, F_SUB, F_SUB_NARROW, F_SUBG, F_FUSED, F_FUSEDW, F_IN2, F_IN2_SUB, F_DIST, F_DIST_SUB,
                F_XV, F_XV_FUSED, F_XV_SUB, F_XV_SUBG };
static const char* const conv_form_name[] = {"plain", "narrow", "slim", "sub", "sub_narrow", "subg", "fused", "fusedw", "in2", "in2_sub",
                                             "dist", "dist_sub", "xv", "xv_fused", "xv_sub", "xv_subg"};

// The instance of family `form` with K taps per phase at tile (TM, TN): kernel (null: none instantiated), reduction block, staging depth
// (CB == 0: no instance at all for K taps).
struct ConvInstance {
    conv_kernel_fn fn;
    int CB, nx;
};
static ConvInstance conv_instance(ConvForm form, int K, int TM, int TN) {
    ConvInstance r{nullptr, 0, 0};
    switch (K) {
#define X(k) case k: r.CB = conv_kernel_cb_k##k(); r.nx = conv_kernel_nx_k##k(); if (form == F_PLAIN) r.fn = conv_kernel_table_k##k(TM, TN); break;
        NC_K_CASES(X)
#undef X
    }
#define X(f, k, name, args, cb, nx_) if (form == F_##f && K == k) { r.fn = conv_kernel_table_##name(NC_TABLE_CALL_##args); if (cb) { r.CB = cb; r.nx = nx_; } }
    NC_CONV_FAMILIES(X)
#undef X
    return r;
}
// reduction block / staging depth of the plain instances with K taps per phase (the packing and the tile rules work from these)
static ConvInstance plain_geometry(int K) {
    const ConvInstance r = conv_instance(F_PLAIN, K, 0, 0);
    if (!r.CB) fail(NC_EUNSUPPORTED, "convolution with %d taps per phase has no kernel instantiation", K);
    return r;
}

// column tiles of `bn` columns over B clips of `cols` columns each: per clip, or over the flattened (clip, column) axis
static int64_t col_tiles(int64_t B, int64_t cols, int64_t bn, bool flat) { return flat ? (B * cols + bn - 1) / bn : B * ((cols + bn - 1) / bn); }

// Everything launch_conv decides for a launch of the windowed template, made by plan_conv_template without a HIP call.
struct ConvPlan {
    conv_kernel_fn fn = nullptr;
    int64_t grid = 0;
    int threads = 0;
    size_t lds = 0;        // dynamic LDS bytes
    ConvArgs a{};
    TileCfg c{};           // TM, TN, NW, CB (and K = taps per phase) of the instance
    int nx = 0;            // staging registers per lane the instance was compiled with
    bool flat = false, narrow = false, slim = false, dist = false, xv = false, fused_wide = false;
    const char* form = "";
    // geometry the steps hand on
    int in_mode = 0, sx = 1, ad = 1;     // x step per output column, |tap step|
    int64_t n_cols = 0, Tout = 0;        // columns per clip of the launch (per phase), output samples per row
    int flat_S = 0, flat_hc = 0;         // flattened axis: clips a tile can touch, halo columns per clip
    int64_t flat_pitch = 0;              // columns per clip on the flattened axis (>= n_cols)
    int xv_extra = 0;                    // slots the window start moves left to land on a vector boundary

    int64_t col_tiles_of(int B, int64_t bn) const { return col_tiles(B, flat ? flat_pitch : n_cols, bn, flat); }
    // staged window of a tile of `cols` columns (+ `halo` halo columns of further clips), in slots per channel row
    int window(int64_t cols, int64_t halo = 0) const { return (int)((cols - 1 + halo) * sx + (c.K - 1) * ad + 1); }
    // ... and whether `nw` waves hold it in their staging registers
    bool window_fits(int xw, int nw) const { return c.CB * ((xw + 63) / 64) <= nw * nx; }
};

}  // namespace nc
