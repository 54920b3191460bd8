// Host side of the implicit-GEMM convolution: weight packing, launch planning, launch.  launch_conv, in order:
//   1. input checks
//   2. the special kernels, each tried in turn and falling through when its launcher declines: skinny projection, thin head in the
//      Encodec input mode, thin head, stem, short-row kernel, pointwise kernel, streaming k = 3
//   3. plan_conv_template (no HIP call): row tile, column tile, narrow, flattened axis, 128-column tiles by rounds, slim, distributed,
//      arguments, XV grant, window geometry, LDS, instance (conv_instance)
//   4. one launch block: dynamic-LDS opt-in, profiler, launch, trace, log
#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <set>

#include "nc_conv.h"
#include "nc_conv_plan.h"
#include "nc_limits.h"

namespace nc {

conv_kernel_fn conv1x1_kernel_table(int, int);
bool launch_conv_thin(const float* x, int64_t x_bstride, int64_t x_cstride, int Cin, int x_len, const float* w_dense, const float* bias, float* y,
                      int64_t y_bstride, int64_t y_cstride, int B, int Cout, int K, int pad, int dil, int64_t Tout, bool tanh_out, hipStream_t s);
bool launch_conv_stem(const float* x, int64_t x_bstride, int x_len, const float* w_dense, const float* bias, const float* alpha_out, float* y,
                      int64_t y_bstride, int64_t y_cstride, int B, int Cout, int K, int pad, int64_t Tout, hipStream_t s);
void launch_skinny_proj(const float* x, int64_t x_bstride, int64_t x_cstride, const float* wp, const float* bias, float* y, int64_t y_bstride,
                        int64_t y_cstride, int B, int Cin, int Cout, int64_t T, hipStream_t s);

// exact small-range division by multiplication: n / d == (n * magic) >> 20 for all 0 <= n < limit
static int32_t magic_div(int d, int limit) {
    const int32_t m = (int32_t)(((1u << 20) + d - 1) / d);
    for (int n = 0; n < limit; ++n)
        if ((int)(((int64_t)n * m) >> 20) != n / d || (int64_t)n * m > 0x7fffffffLL)
            fail(NC_EUNSUPPORTED, "internal: no exact reciprocal for /%d below %d", d, limit);
    return m;
}

TileCfg pick_tile(int Cout, int Ktaps) {
    TileCfg c{};
    int best = 1 << 30;
    for (int tm = 4; tm >= 1; --tm) {
        int bm = 32 * tm;
        int padded = (Cout + bm - 1) / bm * bm;
        if (padded < best) {
            best = padded;
            c.TM = tm;
        }
    }
    if (const int tm = (int)env_int("NC_TM_FORCE", 0)) {   // experiment: force the row-tile height where it divides Cout
        if (tm >= 1 && tm <= 4 && Cout % (32 * tm) == 0) c.TM = tm;
    }
    c.TN = 2;
    c.K = Ktaps;
    c.CB = plain_geometry(Ktaps).CB;
    return c;
}

int64_t ConvLayer::out_len(int64_t Tin) const {
    if (transposed) return (Tin - 1) * stride - 2 * (int64_t)pad + K + out_pad;
    return (Tin + 2 * (int64_t)pad - (int64_t)dil * (K - 1) - 1) / stride + 1;
}

double ConvLayer::flops(int B, int64_t Tin) const {
    if (transposed) return 2.0 * Cin * Cout * K * (double)Tin * B;  // counted on L_in
    return 2.0 * Cin * Cout * K * (double)out_len(Tin) * B;
}

void ConvLayer::build(const float* dense_w, const float* bias_h, int Cin_, int Cout_, int K_, int stride_, int pad_, int dil_,
                      int out_pad_, bool transposed_) {
    Cin = Cin_; Cout = Cout_; K = K_; stride = stride_; pad = pad_; dil = dil_; out_pad = out_pad_; transposed = transposed_;
    sub_shift = 0;
    sub_stride = 0;
    if (transposed) {
        if (dil != 1) fail(NC_EUNSUPPORTED, "dilated conv_transpose1d is not on the hot path");
        n_phase = stride;
        Ktaps = (K + stride - 1) / stride;
        // sub-pixel form (one launch, rows = (channel, phase)): power-of-two strides with two taps per phase, i.e. the k = 2s
        // up-convolutions of DAC / SNAC (DecoderBlock.cs:27-33); other strides keep the per-phase launches
        static const bool no_sub = env_flag("NC_NO_SUBPIXEL");
        if (!no_sub && (stride == 2 || stride == 4 || stride == 8) && K == 2 * stride && (Cout * stride) % 32 == 0 && out_pad == 0) {
            sub_shift = stride == 2 ? 1 : stride == 4 ? 2 : 3;
            sub_stride = stride;
            n_phase = 1;
        }
        // ... and the same form for the other strides (SNAC's stride-3 and Encodec's stride-5 up-convolutions, k = 2s): one launch with
        // full row tiles instead of s launches that each write every s-th sample (NC_NO_SUBPIXEL_ANY=1: per-phase launches)
        static const bool no_sub_any = env_flag("NC_NO_SUBPIXEL_ANY");
        // (output_padding -- stride % 2 in SNAC's DecoderBlock -- only moves the right crop: the extra samples lie inside the (Tin + 1) * s
        // samples the rows cover as long as out_pad <= pad, and the store bounds come from out_len())
        if (!no_sub && !no_sub_any && !sub_stride && stride >= 3 && stride <= 16 && K == 2 * stride && (Cout * stride) % 32 == 0 && out_pad <= pad) {
            sub_stride = stride;
            n_phase = 1;
        }
    } else {
        if (stride > 1 && dil != 1) fail(NC_EUNSUPPORTED, "strided+dilated conv1d is not on the hot path");
        n_phase = 1;
        Ktaps = K;
    }
    cfg = pick_tile(rows(), Ktaps);
    auto pack = [&](const TileCfg& tc, DevBuf& dstbuf, int64_t& phase_stride) {
        const int BM = tc.BM(), CB = tc.CB, KB = tc.KB();
        const int n_co = (rows() + BM - 1) / BM;
        const int n_cb = (Cin + CB - 1) / CB;
        phase_stride = (int64_t)n_co * n_cb * KB * BM;
        std::vector<float> packed((size_t)phase_stride * n_phase, 0.0f);
        for (int ph = 0; ph < n_phase; ++ph)
            for (int ct = 0; ct < n_co; ++ct)
                for (int cb = 0; cb < n_cb; ++cb) {
                    float* dst = packed.data() + (size_t)ph * phase_stride + ((size_t)ct * n_cb + cb) * KB * BM;
                    for (int kk = 0; kk < KB; ++kk) {
                        const int ci = cb * CB + kk / Ktaps, k = kk % Ktaps;
                        if (ci >= Cin) continue;
                        for (int r = 0; r < BM; ++r) {
                            int co = ct * BM + r, php = ph;
                            if (co >= rows()) continue;
                            if (sub_stride) { php = co % stride; co /= stride; }   // row = co*stride + phase
                            float v;
                            if (transposed) {
                                const int kt = php + k * stride;  // tap of this phase, ascending (canonical order)
                                if (kt >= K) continue;
                                v = dense_w[((size_t)ci * Cout + co) * K + kt];
                            } else {
                                v = dense_w[((size_t)co * Cin + ci) * K + k];
                            }
                            dst[(size_t)kk * BM + a_tile_pos(tc.TM, r / 32, r % 32)] = v;
                        }
                    }
                }
        dstbuf.reserve(packed.size() * sizeof(float));
        NC_HIP(hipMemcpy(dstbuf.p, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice));
    };
    pack(cfg, w, w_phase_stride);
    alts.clear();
    static const bool no_alts = env_flag("NC_NO_TILE_ALTS");
    if (!no_alts && rows() >= 128)
        for (int tm = 3; tm >= 1; --tm) {   // (single-row-block tiles: slower on every filled grid, chosen only for the tiny grids of choose_tile)
            if (tm == cfg.TM || rows() % (32 * tm) != 0) continue;
            alts.emplace_back(new Alt());
            alts.back()->cfg = cfg;
            alts.back()->cfg.TM = tm;
            pack(alts.back()->cfg, alts.back()->w, alts.back()->w_phase_stride);
        }
    // whole-channel tile of the wide fused residual units (C = 192 / 256 -> TM = 6 / 8; launched only through ConvIO::fuse_k1)
    static const bool no_wide_fuse = env_flag("NC_NO_WIDE_FUSE");
    const bool wide_c = Cin == Cout && (Cout == 256 || Cout == 192);
    if (!no_alts && !no_wide_fuse && !transposed && K == 7 && stride == 1 && wide_c) {
        alts.emplace_back(new Alt());
        alts.back()->cfg = cfg;
        alts.back()->cfg.TM = Cout / 32;
        pack(alts.back()->cfg, alts.back()->w, alts.back()->w_phase_stride);
    }
    if (!transposed && K == 1 && Cin == Cout && Cin % 32 == 0 && (Cin <= 128 || (wide_c && !no_wide_fuse))) {
        // image for the fused residual-unit tail: [row block][ci][32 rows]
        std::vector<float> f((size_t)Cin * Cout);
        for (int i2 = 0; i2 < Cout / 32; ++i2)
            for (int ci = 0; ci < Cin; ++ci)
                for (int rr = 0; rr < 32; ++rr) f[((size_t)i2 * Cin + ci) * 32 + rr] = dense_w[(size_t)(i2 * 32 + rr) * Cin + ci];
        w_fused.reserve(f.size() * sizeof(float));
        NC_HIP(hipMemcpy(w_fused.p, f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    if (!transposed && K == 1 && Cout <= 16 && Cin % 64 == 0) {
        // image for skinny_proj_kernel: lane = (k4 << 4) | row, value W[row][4*kp + k4]
        std::vector<float> f((size_t)Cin * 16, 0.0f);
        for (int kp = 0; kp < Cin / 4; ++kp)
            for (int l = 0; l < 64; ++l) {
                const int k4 = l >> 4, r = l & 15;
                if (r < Cout) f[(size_t)kp * 64 + l] = dense_w[(size_t)r * Cin + 4 * kp + k4];
            }
        w_skinny.reserve(f.size() * sizeof(float));
        NC_HIP(hipMemcpy(w_skinny.p, f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    if (!transposed && stride == 1 && dil == 1 && Cin == 1 && K == 7) {   // dense [Cout][1][K] image for the streaming stem kernel
        w_stem.reserve(sizeof(float) * (size_t)Cout * K);
        NC_HIP(hipMemcpy(w_stem.p, dense_w, sizeof(float) * (size_t)Cout * K, hipMemcpyHostToDevice));
    }
    {   // image for the short-row kernel (nc_conv_small.hip): the strided down-convolutions, taken when a launch has few columns
        static const bool no_small = env_flag("NC_NO_CONV_SMALL");
        if (!no_small && conv_small_eligible(Cin, Cout, K, stride, dil, transposed)) {
            std::vector<float> img;
            pack_conv_small(dense_w, Cin, Cout, K, img);
            w_small.reserve(img.size() * sizeof(float));
            NC_HIP(hipMemcpy(w_small.p, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice));
        }
    }
    if (!transposed && stride == 1 && Cout <= 2 && (K == 7 || K == 3 || K == 1)) {
        w_thin.reserve(sizeof(float) * (size_t)Cout * Cin * K);
        NC_HIP(hipMemcpy(w_thin.p, dense_w, sizeof(float) * (size_t)Cout * Cin * K, hipMemcpyHostToDevice));
    }
    has_bias = bias_h != nullptr;
    if (has_bias) {
        bias.reserve(sizeof(float) * Cout);
        NC_HIP(hipMemcpy(bias.p, bias_h, sizeof(float) * Cout, hipMemcpyHostToDevice));
    }
}

bool can_fuse_res_unit(const ConvLayer& k7, const ConvLayer& k1) {
    bool tile = k7.Cout <= 128;
    for (const auto& a : k7.alts) tile = tile || a->cfg.BM() == k7.Cout;   // wide units: the whole-channel tile was packed at load
    return !k7.transposed && k7.K == 7 && k7.stride == 1 && k7.Cin == k7.Cout && k7.Cout % 32 == 0 && k7.Cout >= 64 && tile &&
           k1.K == 1 && k1.Cin == k7.Cout && k1.Cout == k7.Cout && k1.w_fused.p != nullptr &&
           k7.has_bias && k1.has_bias;
}


// ---- small answers every path shares ----------------------------------------------------------------------------------------
// ConvArgs::in_mode of a launch: bit 0 pending GroupNorm, bit 1 ELU, bit 2 reflect-padded view, bit 3 second operand
static int in_mode_of(const ConvIO& io) { return (io.in_stats ? 1 : 0) | (io.in_elu ? 2 : 0) | (io.in_L > 0 ? 4 : 0) | (io.x2 ? 8 : 0); }
// the multiply-shift sub-pixel form (strides that are no power of two)
static bool subg_layer(const ConvLayer& L) { return L.sub_stride && !L.sub_shift; }
// family of the two-input (ConvIO::x2) instances of a layer (the multiply-shift sub-pixel form has none)
static ConvForm in2_form(const ConvLayer& L) { return L.sub_shift ? F_IN2_SUB : F_IN2; }
static int row_tiles(const ConvLayer& L, const TileCfg& c) { return (L.rows() + c.BM() - 1) / c.BM(); }
// workgroups of the windowed template resident per CU, by row-tile height TM
static const int bpc_gen[5] = {0, 4, 3, 2, 2};
static bool aligned_to(const void* q, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(q) & (bytes - 1)) == 0; }

// XV staging reads the window in whole words of `vw` floats: plain input (nothing pending on it, no second operand, no GroupNorm sums
// out) whose rows all start on 64-byte boundaries.  (k = 7: the XV-only instances are worth 1.4-2.9 % per layer wherever the rows start
// on 64-byte boundaries (row pitch a multiple of 16 samples) and LOSE 25 % where they do not: C = 768 at 696 steps (2784-byte rows: every
// other channel row starts 32 bytes into a 64-byte sector) 1632 -> 2038 us, at 704 steps 1601 -> 1577, at 1024 2104 -> 2041, at 5568
// 11 254 -> 10 943 (tools/probe/xvk7_rows.py, profiles/r05_xvk7_rows.txt): the 8-byte vector loads are that sensitive, the legacy dword
// loads are not.)
static bool xv_input_ok(const ConvIO& io, int vw) {
    return !in_mode_of(io) && !io.gn_part && io.x_len % vw == 0 && io.x_cstride % 16 == 0 && io.x_bstride % 16 == 0 && aligned_to(io.x, 64);
}
// layers of the two-tap sub-pixel XV instances (4-float words); their remaining conditions depend on the tile (plan_xv)
static bool xv_two_tap_layer(const ConvLayer& L, const ConvIO& io) { return L.sub_stride && L.n_phase == 1 && !io.alpha_in && !io.fuse_k1; }

// Which packed row-tile height to launch: estimated time = rounds * (blocks per CU) * TM * penalty(TM), with
// rounds = ceil(blocks / (256 CUs * blocks per CU)).  Smaller tiles waste a little more LDS/issue bandwidth per MFMA (penalty) but
// can turn a 1.1-round grid into a full one (measured: C=768 at T=696 76 -> 99 TFLOP/s with 96-row tiles).
struct TileChoice {
    TileCfg cfg;
    const float* w;
    int64_t w_phase_stride;
};
static TileChoice choose_tile(const ConvLayer& L, int64_t blocks_per_rowtile, bool pointwise_fast, bool xv_cand = false) {
    auto cost = [&](const TileCfg& c) {
        const double blocks = (double)blocks_per_rowtile * row_tiles(L, c);
        static const int bpc_pw[5] = {0, 6, 5, 3, 3};
        static const double pen_gen[5] = {0, 1.30, 1.10, 1.05, 1.00};
        // pointwise kernel (re-fitted in round 4 after its ring / addressing changes: 96-row tiles are now its most efficient -- C = 384
        // over 32 x 5568 columns 460 us with 128-row tiles, 427 with 96)
        static const double pen_pw[5] = {0, 1.30, 1.10, 1.02, 1.06};
        const double* pen = pointwise_fast ? pen_pw : pen_gen;
        const int bpc = pointwise_fast ? bpc_pw[c.TM] : bpc_gen[c.TM];
        const double rounds = std::ceil(blocks / (256.0 * bpc));
        // (k = 7 at 128 rows x 256 columns runs out of registers -- 212 B of scratch per lane; C = 256: 1.80 ms against 1.65 ms with 64-row tiles)
        double inst = (c.TM == 4 && c.K == 7 && !pointwise_fast) ? 1.12 : 1.0;
        // Two-tap sub-pixel up-convolutions with SHORT reductions (Cin <= 384: 12-24 reduction blocks per tile): a tile's prologue and
        // epilogue -- an output-heavy epilogue: stride x more samples out than in -- are 10-15 % of its life, and the 64-row instance is the
        // only one of the three that does not spill (241 registers; 96 rows: 256 + 26 spilled, 128 rows: 256 + 136).  Measured with the XV
        // staging (tools/probe/tm_pick_up.sh, one box): 192 -> 96 at 32 x 22 272 columns 1079 us with 96-row tiles, 980 with 64-row tiles
        // (SNAC's at 8 x 110 592: 1318 / 1200); 384 -> 192: 1943 / 1834; from 768 input channels on the 96-row tiles win (2119 / 2215).
        static const bool xv_off = env_flag("NC_NO_XV") || env_flag("NC_NO_XR");   // (the legacy 64-row instance does not win: conv_up 5.94 -> 6.15 ms)
        if (xv_cand && !xv_off && L.sub_stride && c.K == 2 && c.TM == 2 && L.Cin <= 384) inst = 0.88;   // (xv_cand: this launch takes the XV-only instance)
        return rounds * bpc * c.TM * pen[c.TM] * inst;
    };
    TileChoice best{L.cfg, L.w.as<float>(), L.w_phase_stride};
    double bc = cost(L.cfg);
    {   // Tiny grids (one-clip / short-row launches: even with 32-row tiles every workgroup gets a CU of its own): a workgroup's life is
        // its serial reduction, TM matrix-core chains long per step, so the SMALLEST row tile finishes first -- SNAC 24 kHz at one clip:
        // the 384 -> 768 k=16 down-convolution ran 8 workgroups of 96 rows for 450 us (C1: 2.85 ms in all).
        static const bool no_tiny = env_flag("NC_NO_TINY_TILES");
        static const int tiny_blocks = (int)env_int("NC_TINY_BLOCKS", 256);
        if (!no_tiny) {
            // the smallest packed row tile whose grid still stays under `tiny_blocks` workgroups
            int tm = 0;
            for (int cand = 1; cand < L.cfg.TM && !tm; ++cand) {
                if (blocks_per_rowtile * ((L.rows() + 32 * cand - 1) / (32 * cand)) > tiny_blocks) continue;
                for (const auto& a : L.alts)
                    if (a->cfg.TM == cand) { tm = cand; best = TileChoice{a->cfg, a->w.as<float>(), a->w_phase_stride}; }
            }
            if (tm) return best;
        }
    }
    static const int tm_pick = (int)env_int("NC_TM_PICK", 0);   // experiment: force a packed variant
    if (tm_pick) {
        for (const auto& a : L.alts)
            if (a->cfg.TM == tm_pick && tm_pick <= 4) return TileChoice{a->cfg, a->w.as<float>(), a->w_phase_stride};
        return best;
    }
    for (const auto& a : L.alts) {
        if (a->cfg.TM > 4 || a->cfg.TM == 1) continue;   // whole-channel tiles of the wide fused units; 32-row tiles: tiny grids only (above)
        const double c = cost(a->cfg);
        if (c < bc) {
            bc = c;
            best = TileChoice{a->cfg, a->w.as<float>(), a->w_phase_stride};
        }
    }
    return best;
}

// Row tiles per group of the block -> tile order (ConvArgs::co_group).  The ~64 workgroups resident on an XCD advance through their
// reduction blocks roughly in step, so operands they have in common are fetched from the fabric once and then hit in that XCD's L2
// (temporal sharing: the instantaneous working set is a few tiles, far below the 4 MB).  With groups of G row tiles the resident set
// is G row tiles x 64/G column tiles: an input window is fetched once per GROUP (x_bytes * n_co / G in all) and a weight panel once per
// resident set that holds it (w_bytes * n_col_tiles * G / 64 in all).  Pick the divisor of n_co_tiles (<= 8) with the least traffic.
// Measured (PMC FETCH_SIZE, DAC C2): G = 1 -> 2 on the C = 384 k = 7 layers 1156 -> 709 MiB per launch, as this model predicts.
// NC_CO_GROUP=<n> caps the group size (1 = one panel per XCD, the round-1 order).
static int pick_co_group(int n_co_tiles, double x_bytes, double w_bytes, double n_col_tiles) {
    static const int cap = (int)env_int("NC_CO_GROUP", 0);
    int best = 1;
    double bt = 0.0;
    for (int g = 1; g <= std::min(n_co_tiles, cap > 0 ? cap : 8); ++g) {
        if (n_co_tiles % g) continue;
        const double t = x_bytes * n_co_tiles / g + w_bytes * n_col_tiles * g / 64.0;
        if (g == 1 || t < bt) { bt = t; best = g; }
    }
    return best;
}

static const float* bias_of(const ConvLayer& L) { return L.has_bias ? L.bias.as<float>() : nullptr; }
// the ConvArgs fields every kernel of this file takes as the caller gave them: input, output, bias, pending GroupNorm of the input (mode
// bits 0-1), GroupNorm block sums of the output
static ConvArgs conv_args_io(const ConvLayer& L, const ConvIO& io, const float* w) {
    ConvArgs a{};
    a.x = io.x; a.x_bstride = io.x_bstride; a.x_cstride = io.x_cstride; a.Cin = L.Cin; a.x_len = io.x_len;
    a.w = w;
    a.bias = bias_of(L);
    a.y = io.y; a.y_bstride = io.y_bstride; a.y_cstride = io.y_cstride;
    a.in_mode = in_mode_of(io) & 3; a.in_stats = io.in_stats; a.in_gamma = io.in_gamma; a.in_beta = io.in_beta;
    a.gn_part = io.gn_part; a.gn_nrb = io.gn_nrb; a.gn_ncb = io.gn_ncb; a.gn_count = io.gn_count; a.gn_stats = io.gn_stats; a.gn_n = io.gn_n;
    return a;
}
// activations in and out plus the weights, in bytes: the traffic figure the profiler gets for a launch
static double conv_bytes(const ConvLayer& L, int B, double cols_in, double cols_out) {
    return 4.0 * ((double)B * L.Cin * cols_in + (double)B * L.Cout * cols_out + (double)L.Cin * L.Cout * L.K);
}

// NC_LAUNCH_LOG=<path>, one "conv_plan" line per launch_conv call: the form, the kernel's symbol as the runtime names the pointer, grid,
// threads and dynamic LDS bytes ("- 0 0 0" where the launcher of another unit chose them), then the template's decisions (log_plan).
static void log_form(FILE* lf, const char* form, const void* fn, hipStream_t stream, int64_t grid, int threads, size_t lds) {
    const char* sym = fn ? hipKernelNameRefByPtr(fn, stream) : "-";
    std::fprintf(lf, "conv_plan %s %s %lld %d %zu", form, sym ? sym : "?", (long long)grid, threads, lds);
}
static void log_special(const char* form, const void* fn = nullptr, hipStream_t stream = nullptr, int64_t grid = 0, int threads = 0) {
    FILE* lf = launch_log();
    if (!lf) return;
    log_form(lf, form, fn, stream, grid, threads, 0);
    std::fputc('\n', lf);
    std::fflush(lf);
}

// ---- the special kernels ----------------------------------------------------------------------------------------------------
// The two kernels that take their B fragments straight from global memory (256-column tiles over T columns per clip, 16-channel
// reduction blocks, no LDS window): tile map, profiler, launch.
static void launch_direct(const char* form, conv_kernel_fn fn, ConvArgs& a, const ConvLayer& L, const TileChoice& tc, int B, int64_t T,
                          double flops, double bytes, hipStream_t stream, Profiler* prof) {
    a.Cout = L.Cout; a.B = B; a.Tout = (int32_t)T;
    a.n_co_tiles = row_tiles(L, tc.cfg);
    a.n_t_tiles = (int32_t)col_tiles(1, T, 256, false);
    a.n_cb = (L.Cin + 15) / 16;
    a.co_group = pick_co_group(a.n_co_tiles, 4.0 * B * L.Cin * (double)T, 4.0 * L.K * L.Cin * (double)L.Cout, (double)B * a.n_t_tiles);
    const int64_t grid = (int64_t)a.n_co_tiles * B * a.n_t_tiles;
    {
        ProfScope ps(prof, stream, L.kclass, flops, bytes);
        hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(256), 0, stream, a);
        NC_HIP(hipGetLastError());
    }
    log_special(form, (const void*)fn, stream, grid, 256);
}

// Streaming k = 3 path of the Encodec residual branches (nc_conv3s.hip): reflect pad 1 + 1 of SConv1d folded into the lane exchange,
// pending GroupNorm + ELU applied once per element in registers, no LDS for the activations.
conv_kernel_fn conv3_stream_kernel_table(int, bool);
static bool launch_conv3_stream(const ConvLayer& L, const ConvIO& io, int B, hipStream_t stream, Profiler* prof) {
    static const bool off = env_flag("NC_NO_CONV3S");
    if (off || L.transposed || L.K != 3 || L.stride != 1 || L.dil != 1 || L.pad != 0 || L.cfg.CB != 16 || (L.Cin & 1) || L.Cin > 512) return false;
    if (io.alpha_in || io.alpha_out || io.res || io.epi || io.fuse_k1 || io.x2 || io.noise) return false;
    // the Encodec input mode with the non-causal pad of a k = 3, stride 1 SConv1d: one reflected sample on either side, no zero extension
    const int64_t T = io.in_L;
    if (T < 4 || (T & 1) || io.in_left != 1 || io.in_Lz != T || io.Tin != T + 2 || io.x_len != T + 2) return false;
    if ((io.y_cstride & 1) || (io.y_bstride & 1)) return false;
    if (!aligned_to(io.y, 8)) return false;
    const bool x_aligned = aligned_to(io.x, 8) && !(io.x_cstride & 1) && !(io.x_bstride & 1);
    if ((int64_t)(L.Cin + 1) * io.x_cstride + T >= ((int64_t)1 << 32)) return false;
    const TileChoice tc = choose_tile(L, col_tiles(B, T, 256, false), true);
    conv_kernel_fn fn = conv3_stream_kernel_table(tc.cfg.TM, x_aligned);
    if (!fn) return false;
    ConvArgs a = conv_args_io(L, io, tc.w);
    a.x_len = (int32_t)T;
    launch_direct("k3_stream", fn, a, L, tc, B, T, 2.0 * L.Cin * L.Cout * 3 * (double)T * B,
                  4.0 * ((double)B * L.Cin * T + (double)B * L.Cout * T + 3.0 * L.Cin * L.Cout), stream, prof);
    return true;
}

// Pointwise fast path (nc_conv1x1.hip): B fragments straight from global memory, 2-wide vector loads/stores.
static bool launch_conv1x1(const ConvLayer& L, const ConvIO& io, int B, hipStream_t stream, Profiler* prof) {
    static const bool off = env_flag("NC_NO_CONV1X1");
    const int64_t T = io.Tin;
    if (off || L.transposed || L.K != 1 || L.stride != 1 || L.pad != 0 || L.cfg.CB != 16 || io.fuse_k1 || (L.Cin & 1)) return false;
    if (io.alpha_in || (io.epi & ~EPI_NOISE) || T < 2 || (T & 1) || io.x_len != T) return false;
    if (io.alpha_out && (io.epi & EPI_NOISE)) return false;
    if ((io.x_cstride & 1) || (io.x_bstride & 1) || (io.y_cstride & 1) || (io.y_bstride & 1)) return false;
    if ((int64_t)L.Cin * io.x_cstride * 4 >= ((int64_t)1 << 32)) return false;   // (the B reads are buffer loads over one clip's rows)
    if (!aligned_to(io.x, 8) || !aligned_to(io.y, 8) || (io.res && !aligned_to(io.res, 8)) || (io.noise && !aligned_to(io.noise, 8))) return false;
    if ((io.epi & EPI_NOISE) && (!io.noise || !io.res)) return false;
    const int in_mode = in_mode_of(io) & 3;
    if (io.in_L > 0 || io.x2) return false;   // (reflect addressing / two operands: the windowed template)
    if (in_mode && (io.res || io.alpha_out || io.epi || L.Cin > 512)) return false;
    const TileChoice tc = choose_tile(L, col_tiles(B, T, 256, false), true);
    const int mode = in_mode ? 8 : (io.epi & EPI_NOISE) ? 4 : ((io.res ? 1 : 0) | (io.alpha_out ? 2 : 0));
    if (io.gn_part && mode != 8) return false;   // block sums are emitted by the input-mode instance only (the windowed template has them everywhere)
    conv_kernel_fn fn = conv1x1_kernel_table(tc.cfg.TM, mode);
    if (!fn) return false;
    ConvArgs a = conv_args_io(L, io, tc.w);
    a.res = io.res; a.noise = io.noise; a.noise_bstride = T; a.epi = io.epi; a.alpha_out = io.alpha_out;
    launch_direct("pointwise", fn, a, L, tc, B, T, L.flops(B, T),
                  4.0 * ((double)B * L.Cin * T + (double)B * L.Cout * T * (io.res ? 2 : 1) + (double)L.Cin * L.Cout), stream, prof);
    return true;
}

// skinny projections (Cout <= 16: the quantizer's in_proj): one streaming kernel, plain input and epilogue only
static bool launch_skinny(const ConvLayer& L, const ConvIO& io, int B, hipStream_t stream, Profiler* prof) {
    static const bool no_skinny = env_flag("NC_NO_SKINNY");
    if (!L.w_skinny.p || no_skinny || in_mode_of(io) || io.alpha_in || io.alpha_out || io.res || io.epi != 0 || io.fuse_k1 || io.x_len != io.Tin) return false;
    ProfScope ps(prof, stream, L.kclass, L.flops(B, io.Tin), conv_bytes(L, B, (double)io.Tin, (double)io.Tin));
    launch_skinny_proj(io.x, io.x_bstride, io.x_cstride, L.w_skinny.as<float>(), bias_of(L), io.y, io.y_bstride, io.y_cstride, B, L.Cin, L.Cout, io.Tin, stream);
    return true;
}

// thin-output layers the input-mode streaming kernel serves: Conv1d(C -> 1|2, k = 7), stride 1, no dilation, explicit padding
static bool thin_inm_layer(const ConvLayer& L) {
    static const bool off = env_flag("NC_NO_THIN_INM");
    return !off && L.w_thin.p && !L.transposed && L.K == 7 && L.stride == 1 && L.dil == 1 && L.pad == 0 && L.Cout <= 2;
}

// the PCM head in the Encodec input mode: both operands, normalise + add + ELU + reflect pad while staging, GroupNorm sums of the output
static bool launch_thin_inm(const ConvLayer& L, const ConvIO& io, int B, hipStream_t stream, Profiler* prof) {
    if (!thin_inm_layer(L) || io.in_L <= 0 || io.alpha_in || io.alpha_out || io.res || io.fuse_k1 || io.epi != 0 ||
        (io.x2 && (io.in_stats != nullptr) != (io.in_stats2 != nullptr)))
        return false;
    ThinInmArgs t{};
    t.xa = io.x; t.xb2 = io.x2; t.x_bstride = io.x_bstride; t.x_cstride = io.x_cstride;
    t.Cin = L.Cin; t.L = (int)io.in_L; t.left = (int)io.in_left; t.Lz = (int)io.in_Lz; t.Lp = (int)io.Tin;
    t.stats_a = io.in_stats; t.gamma_a = io.in_gamma; t.beta_a = io.in_beta;
    t.stats_b = io.in_stats2; t.gamma_b = io.in_gamma2; t.beta_b = io.in_beta2;
    t.elu = io.in_elu ? 1 : 0;
    t.w = L.w_thin.as<float>(); t.bias = bias_of(L);
    t.y = io.y; t.y_bstride = io.y_bstride; t.y_cstride = io.y_cstride;
    t.Tout = (int)L.out_len(io.Tin);
    t.gn_part = io.gn_part; t.gn_ncb = io.gn_ncb; t.gn_count = io.gn_count; t.gn_stats = io.gn_stats; t.gn_n = io.gn_n;
    if (io.gn_part && io.gn_nrb != 1) fail(NC_ESTATE, "internal: thin head with more than one GroupNorm row block");
    ProfScope ps(prof, stream, L.kclass, L.flops(B, io.Tin),
                 4.0 * ((double)B * L.Cin * io.in_L * (io.x2 ? 2 : 1) + (double)B * L.Cout * t.Tout + (double)L.Cin * L.Cout * L.K));
    return launch_conv_thin_inm(t, B, L.Cout, stream);
}

// thin-output layers (PCM heads): streaming kernel instead of a 32-row matrix tile with 1-2 live rows
static bool launch_thin(const ConvLayer& L, const ConvIO& io, int B, hipStream_t stream, Profiler* prof) {
    static const bool no_thin = env_flag("NC_NO_THIN");
    if (!L.w_thin.p || no_thin || in_mode_of(io) || io.alpha_in || io.alpha_out || io.res || io.fuse_k1 || (io.epi & ~EPI_TANH) != 0) return false;
    const int64_t Tout = L.out_len(io.Tin);
    ProfScope ps(prof, stream, L.kclass, L.flops(B, io.Tin), conv_bytes(L, B, (double)io.Tin, (double)Tout));
    return launch_conv_thin(io.x, io.x_bstride, io.x_cstride, L.Cin, io.x_len, L.w_thin.as<float>(), bias_of(L), io.y, io.y_bstride, io.y_cstride,
                            B, L.Cout, L.K, L.pad, L.dil, Tout, (io.epi & EPI_TANH) != 0, stream);
}

// thin-input layers (stems, Cin == 1): streaming store of Cout rows
static bool launch_stem(const ConvLayer& L, const ConvIO& io, int B, hipStream_t stream, Profiler* prof) {
    static const bool no_stem = env_flag("NC_NO_STEM");
    if (!L.w_stem.p || no_stem || in_mode_of(io) || io.alpha_in || io.res || io.fuse_k1 || io.epi != 0 || io.x_cstride < 0) return false;
    const int64_t Tout = L.out_len(io.Tin);
    ProfScope ps(prof, stream, L.kclass, L.flops(B, io.Tin), 4.0 * ((double)B * io.Tin + (double)B * L.Cout * Tout));
    return launch_conv_stem(io.x, io.x_bstride, io.x_len, L.w_stem.as<float>(), bias_of(L), io.alpha_out, io.y, io.y_bstride, io.y_cstride, B, L.Cout,
                            L.K, L.pad, Tout, stream);
}

bool conv_in2_available(const ConvLayer& L) {
    static const bool off = env_flag("NC_NO_IN2");
    if (off || L.w_stem.p || L.w_skinny.p) return false;
    if (L.w_thin.p) return thin_inm_layer(L);   // the PCM head in the input mode takes both operands (conv_thin_inm_kernel)
    // Only where ONE row tile covers all output rows: every row tile re-stages (normalises twice, adds, activates) the window it
    // shares with the others, and on the matrix-core-bound deep layers that vector work sits on the critical path -- measured on C3:
    // 64 -> 128 k8 419 -> 432 us, 128 -> 256 k10 493 -> 1224 us, 256 -> 512 k16 +370 us against the summed copy + one-input launch,
    // while the single-tile layers gain (32 -> 64 k4: 314 -> 275 us, 64 -> 32 up-conv: 368 -> 311 us).
    if (L.rows() > 64 || L.cfg.TM == 3) return false;
    if (subg_layer(L)) return false;   // (the multiply-shift sub-pixel form has no two-input instance)
    return conv_instance(in2_form(L), L.Ktaps, L.cfg.TM, 1).fn != nullptr;
}

// the short-row kernel's instance for this layer and input mode emits GroupNorm block sums from its epilogue
static bool small_emits_gn(const ConvLayer& L, const ConvIO& io) {
    return conv_small_gn_available(L.Cin, L.K, L.stride, L.dil, io.in_stats != nullptr || io.in_elu);
}

// Short-row kernel (nc_conv_small.hip) for this launch?  0 = no, 1 = 16-column tiles (latency-bound launches: few workgroups of any
// shape), 2 = 32-column tiles (k = 16 layers whose template grid would not fill the chip twice: 256 -> 512 at 150 frames x 32 rows
// 365 -> 272 us, 512 -> 1024 at 87 frames x 32 clips 713 -> 572 us; with >= 512 template workgroups the template wins).
static int conv_small_choice(const ConvLayer& L, const ConvIO& io, int B) {
    if (!L.w_small.p || B <= 0) return 0;
    const int in_mode = in_mode_of(io);
    if ((in_mode & 8) || io.alpha_in || io.res || io.fuse_k1 || io.epi != 0) return 0;   // (the reflect-padded view alone is fine: an index map)
    if ((in_mode & 3) && !conv_small_inm_available(L.Cin, L.K, L.stride, L.dil)) return 0;
    static const int64_t max_grid = env_int("NC_SMALL_MAX_GRID", 2048);
    static const int64_t wide_below = env_int("NC_SMALL_WIDE_BELOW", 512);
    const int64_t Tout = L.out_len(io.Tin);
    if (L.K == 1) {   // wide pointwise GEMMs over few columns (the chunked LSTM input projections): 32-column form only
        // (round 6: up to 1024 columns, was 4096 -- every 64-row x 32-column workgroup streams its 128 KB weight panel out of L2, so the 44-step
        //  chunks of C3 (1408 columns: 1408 workgroups, 180 MB of panels, 54 us) run faster on the pointwise kernel's 256-column tiles:
        //  C3 8.47 -> 8.38 ms, C2 53.80 -> 53.67 ms, C5 / C1 unchanged; tools/probe/r6_k1cols2.sh)
        static const int64_t k1_cols = env_int("NC_SMALL_K1_COLS", 1024);
        return (!io.gn_part && (int64_t)B * Tout <= k1_cols) ? 2 : 0;
    }
    const int64_t grid16 = col_tiles(B, Tout, 16, false) * ((L.Cout + 63) / 64);
    if (grid16 <= max_grid) return 1;
    const int64_t template_grid = row_tiles(L, L.cfg) * col_tiles(B, Tout, 256, true);
    if (conv_small_max_tn(L.Cin, L.K, L.stride, L.dil) >= 2 && template_grid < wide_below) return 2;
    return 0;
}

// Short rows of a few-clip batch (one-clip SNAC / DAC: the deep down-convolutions over 47 .. 375 frames) and the k = 16 layers
// whose template grid leaves most of the chip to lone workgroups: the 16x16x4 kernel of nc_conv_small.hip
static bool launch_small(const ConvLayer& L, const ConvIO& io, int B, hipStream_t stream, Profiler* prof) {
    const int small_tn = (!io.gn_part || small_emits_gn(L, io)) ? conv_small_choice(L, io, B) : 0;
    if (!small_tn || (int64_t)(L.Cin) * io.x_cstride + io.x_len >= ((int64_t)1 << 40)) return false;
    const int64_t Tout = L.out_len(io.Tin);
    ProfScope ps(prof, stream, L.kclass, L.flops(B, io.Tin), conv_bytes(L, B, (double)io.Tin, (double)Tout));
    const ConvSmallGn sgn{io.gn_part, io.gn_nrb, io.gn_ncb, io.gn_count, io.gn_stats, io.gn_n};
    return launch_conv_small(io.x, io.x_bstride, io.x_cstride, io.x_len, (int)io.in_left, (int)io.in_Lz, (int)io.in_L, io.in_stats, io.in_gamma, io.in_beta,
                             io.in_elu ? 1 : 0, &sgn, L.w_small.as<float>(), bias_of(L), io.alpha_out, io.y, io.y_bstride, io.y_cstride, B, L.Cin, L.Cout,
                             L.K, L.stride, L.pad, L.dil, (int)Tout, small_tn, stream);
}

bool conv_gn_fusable(const ConvLayer& L, const ConvIO& io, int B) {
    static const bool off = env_flag("NC_NO_GN_FUSE");
    // plain epilogues only; one launch covering the whole output (no per-phase transposed launches); the streaming thin-output /
    // stem / skinny kernels keep the stand-alone statistics pass (launch_conv skips them when gn_part is set, so the answer here only
    // has to say which layers are WORTH routing through the matrix-core template: all but those three)
    if (off || io.res || io.alpha_out || io.alpha_in || io.epi || io.fuse_k1 || L.n_phase != 1 || subg_layer(L)) return false;
    if (L.w_thin.p) return thin_inm_layer(L) && io.in_L > 0;   // (the input-mode head kernel emits its sums; the plain head does not)
    if (L.w_stem.p || L.w_skinny.p) return false;
    // (the short-row kernel's 32-column instances reduce the blocks from an LDS copy of the tile; the others: stand-alone pass)
    return !conv_small_choice(L, io, B) || small_emits_gn(L, io);
}

// ---- the template: plan (ConvPlan: nc_conv_plan.h) -----------------------------------------------------------------------------
// Row tile: the cheapest packed height for the grid (choose_tile), or the whole-channel tile of a fused residual unit.
static TileChoice plan_row_tile(const ConvPlan& p, const ConvLayer& L, const ConvIO& io, int B) {
    TileChoice tsel{L.cfg, L.w.as<float>(), L.w_phase_stride};
    // (launches that will take the XV-only two-tap instance: plain input, rows on 64-byte boundaries; the remaining conditions depend on
    //  the tile and are checked by plan_xv)
    const bool xv_cand = xv_two_tap_layer(L, io) && xv_input_ok(io, 4);
    if (!io.fuse_k1) return choose_tile(L, L.n_phase * col_tiles(B, p.n_cols, 256, false), false, xv_cand);
    for (const auto& alt : L.alts)   // the fused residual unit needs the tile that spans all channels
        if (alt->cfg.BM() == L.Cout) tsel = TileChoice{alt->cfg, alt->w.as<float>(), alt->w_phase_stride};
    return tsel;
}

static void plan_column_tile(ConvPlan& p) {
    static const int tn_thresh = (int)env_int("NC_TN_THRESH", 192);
    p.c.TN = p.n_cols >= tn_thresh ? 2 : 1;  // 256-column tiles for long clips, 128 for the deep (short) layers
    // the per-lane staging registers bound the window: fall back to 128-column tiles when it does not fit
    if (p.c.TN == 2 && !p.window_fits(p.window(p.c.BN()), 4)) p.c.TN = 1;
}

// narrow variant (3 waves, 96 columns): rows of 65..96 columns would leave a quarter of a 128-column tile on padding
static void plan_narrow(ConvPlan& p, const ConvLayer& L, const ConvIO& io) {
    static const bool no_narrow = env_flag("NC_NO_NARROW");
    const int rem = (int)(p.n_cols % 128);
    if (!no_narrow && p.window_fits(p.window(96), 3) && !io.fuse_k1 && !io.x2 && !subg_layer(L) && p.c.TN == 1 && p.n_cols <= 96 && rem > 64 &&
        conv_instance(F_NARROW, p.c.K, p.c.TM, 1).fn) {
        p.narrow = true;
        p.c.NW = 3;
    }
}

// Flattened (clip, column) axis (kernel: "Flattened column axis"): when the rows are short or leave a good part of their last
// tile on padding, the columns of all clips are cut into tiles as one axis.  Needs the one-launch forms (no per-phase launches),
// no per-clip scalars in the kernel (a pending GroupNorm of the Encodec input mode -- measured: per-segment statistics through an LDS table made every
// instance of the template ~5 % slower for 0.07 ms on C3 -- and noise rows), a window (tile + one halo per touched clip) that still fits
// the staging registers, and 32-bit offsets that reach 3 clips ahead.  Picks the row tile again for the flattened grid.
static void plan_flat(ConvPlan& p, TileChoice& tsel, const ConvLayer& L, const ConvIO& io, int B) {
    static const bool no_flat = env_flag("NC_NO_FLAT");
    const int hc = ((L.Ktaps - 1) * p.ad) / p.sx;
    // clip pitch on the flattened axis: the row length, or -- when the epilogue emits GroupNorm block sums -- the row length rounded up
    // to whole 32-column blocks (= 32 * gn_ncb), so that every 32x32 accumulator tile is one canonical block of one sample
    static const bool no_flat_gn = env_flag("NC_NO_FLAT_GN");
    const int64_t Tq = io.gn_part ? (int64_t)32 * io.gn_ncb : p.n_cols;
    auto segs = [&](int BN) { return (int)((BN - 2) / Tq) + 2; };
    auto fits = [&](int TN) {
        const int BN = 128 * TN, S = segs(BN);
        return S <= 4 && p.window_fits(p.window(BN, (S - 1) * hc), 4);
    };
    const bool cand = !no_flat && B > 1 && L.n_phase == 1 && !io.fuse_k1 && !(p.in_mode & 1) && !(io.gn_part && (no_flat_gn || Tq < p.n_cols)) && !io.x2 &&
                      !(io.epi & EPI_NOISE) && Tq >= 32 && L.Cin * L.Ktaps >= 64 &&
                      3 * io.x_bstride + io.x_len < ((int64_t)1 << 32) &&
                      (int64_t)(p.c.BM() + 4) * io.y_cstride + p.Tout + 3 * io.y_bstride < ((int64_t)1 << 31) &&
                      (Tq + hc) * p.sx < (1 << 28);
    int ftn = 0;
    if (cand) ftn = ((int64_t)B * Tq >= 192 && fits(2)) ? 2 : fits(1) ? 1 : 0;
    if (ftn < p.c.TN && p.n_cols >= 192) ftn = 0;   // (dilation-9 windows: the extra halo would halve the tile width -- keep the one-clip tiles)
    if (!ftn) return;
    const int64_t bn_nf = p.c.BN(), cols_nf = col_tiles(B, p.n_cols, bn_nf, false) * bn_nf;
    const int64_t bn_f = 128 * ftn, cols_f = col_tiles(B, Tq, bn_f, true) * bn_f;
    if ((double)cols_f > 0.97 * (double)cols_nf) return;
    p.flat = true;
    tsel = choose_tile(L, col_tiles(B, Tq, 256, true), false);
    p.c = tsel.cfg;
    p.c.TN = ftn;
    p.narrow = false;
    p.flat_S = segs(p.c.BN());
    p.flat_pitch = Tq;
    p.flat_hc = hc;
}

// Small grids of small layers: two 128-column tiles instead of one 256-column tile when that fills the chip better (the
// latency-bound layers of the 1-clip / 150-frame configurations: C1 2.93 -> 2.66 ms, C3 11.66 -> 11.43 ms, Encodec 24 kHz
// 7.05 -> 6.83 ms).  Only where the whole weight set is a few MB: the deep DAC layers stream 16-75 MB of weights per launch and
// a 128-column tile re-reads them twice as often -- there the same switch LOSES 8-23 % (C = 768 k=7 1.74 -> 1.88 ms, up-conv
// 1536->768 1.31 -> 1.62 ms) although the round count says otherwise.
static void plan_tn_rounds(ConvPlan& p, const ConvLayer& L, const ConvIO& io, int B) {
    static const bool no_tn_rounds = env_flag("NC_NO_TN_ROUNDS");
    if (no_tn_rounds || p.c.TN != 2 || io.fuse_k1 || p.narrow || p.c.TM > 4) return;
    const double slots = 256.0 * bpc_gen[p.c.TM];
    const int64_t n_co = row_tiles(L, p.c);
    const double r2 = std::ceil((double)(L.n_phase * n_co * p.col_tiles_of(B, 256)) / slots), r1 = std::ceil((double)(L.n_phase * n_co * p.col_tiles_of(B, 128)) / slots);
    const double w_bytes = 4.0 * L.rows() * (double)L.Cin * L.Ktaps;
    if (r2 <= 3 && r1 * 1.08 < 2.0 * r2 && w_bytes <= 4.0 * 1024 * 1024) {
        p.c.TN = 1;
        if (p.flat) p.flat_S = (int)((128 - 2) / p.flat_pitch) + 2;
    }
}

// Slim variant: half-size reduction block (half the LDS per workgroup), 4+ workgroups per CU.  The narrow long-T layers
// (Cout <= 64: k=3 residual-branch convolutions of the SEANet blocks, the 2-channel Encodec stem) spend their time in memory
// round trips -- two reduction blocks per tile never fill the software pipeline -- so more resident workgroups overlap them:
// 215 -> 145 us (32->16 k3, 48000 steps x 32 clips), 152 -> 118 us (64->32), 80 -> 51 us (2->32 k7).  Measured neutral or
// slower for the strided k=4 / k=8 layers and the sub-pixel up-convolutions, which keep the standard blocks.
static void plan_slim(ConvPlan& p, const ConvLayer& L, const ConvIO& io) {
    static const bool no_slim = env_flag("NC_NO_SLIM");
    if (no_slim || p.flat || p.narrow || io.fuse_k1 || io.x2 || L.sub_stride || L.transposed || p.c.TM > 2 || p.n_cols < 1024) return;
    if (!(p.c.K == 3 && p.c.CB == 16) && !(p.c.K == 7 && p.c.CB == 8 && L.Cin <= 4 && L.stride == 1 && L.dil == 1)) return;
    const ConvInstance s = conv_instance(F_SLIM, p.c.K, p.c.TM, p.c.TN);
    if (s.fn) { p.slim = true; p.c.CB = s.CB; p.nx = s.nx; }
}

// Distributed staging for the grids that leave a workgroup alone on its CU (the deep strided / sub-pixel layers of Encodec at
// 150 frames: 20 GFLOP per launch): nobody feeds the matrix pipe during the staging runs of the segmented pipeline -- measured
// 58 % pipe duty for a lone workgroup against 71 % for a co-resident pair -- so the runs are dealt into the matrix-core shadows.
static ConvForm dist_form(const ConvLayer& L) { return L.sub_shift ? F_DIST_SUB : F_DIST; }
static void plan_dist(ConvPlan& p, const ConvLayer& L, const ConvIO& io, int B) {
    static const bool off = env_flag("NC_NO_DIST_SMALL");
    static const int64_t max_grid = env_int("NC_DIST_MAX_GRID", 768);
    if (off || p.narrow || p.slim || p.in_mode || io.x2 || io.fuse_k1 || io.epi != 0 || L.n_phase != 1 ||
        row_tiles(L, p.c) * p.col_tiles_of(B, p.c.BN()) > max_grid)
        return;
    if ((L.sub_shift && p.c.K == 2) || (!L.sub_stride && !L.transposed && p.c.K == 16))
        p.dist = conv_instance(dist_form(L), p.c.K, p.c.TM, p.c.TN).fn != nullptr;
}

// The argument block but for the window geometry: what the caller handed in, the epilogue, the output map of the (transposed) form.
static void plan_args(ConvPlan& p, const TileChoice& tsel, const ConvLayer& L, const ConvIO& io, int B) {
    ConvArgs& a = p.a;
    a = conv_args_io(L, io, tsel.w);
    a.alpha_in = io.alpha_in;
    a.in_mode = p.in_mode;
    a.x2 = io.x2; a.in_stats2 = io.in_stats2; a.in_gamma2 = io.in_gamma2; a.in_beta2 = io.in_beta2;
    a.in_left = (int32_t)io.in_left; a.in_Lz = (int32_t)io.in_Lz; a.in_L = (int32_t)io.in_L;
    a.w_phase_stride = tsel.w_phase_stride;
    a.alpha_out = io.alpha_out; a.res = io.res;
    a.rvq_zq = io.rvq_zq; a.rvq_res = io.rvq_res;
    a.noise = io.noise; a.noise_bstride = p.Tout;
    if ((io.epi & EPI_NOISE) && (!io.noise || !io.res)) fail(NC_ESTATE, "internal: noise epilogue needs noise and residual");
    a.Cout = L.rows(); a.sub_shift = L.sub_shift; a.B = B; a.epi = io.epi;
    if (subg_layer(L)) {
        if (io.epi & EPI_NOISE) fail(NC_ESTATE, "internal: noise epilogue on the multiply-shift sub-pixel form");
        a.sub_stride = L.sub_stride; a.sub_cout = L.Cout; a.sub_magic = magic_div(L.sub_stride, L.rows() + 256);
        if (!conv_subpixel_fits32(L.Cout, io.y_cstride, io.y_bstride, p.Tout))
            fail(NC_EUNSUPPORTED, "conv output of %lld samples per row exceeds the 32-bit offsets of the sub-pixel form", (long long)io.y_cstride);
    }
    a.Tout = (int32_t)p.Tout;
    if (!conv_rows_fit32(p.c.BM(), io.y_cstride, p.Tout))
        fail(NC_EUNSUPPORTED, "conv output rows of %lld samples exceed the 32-bit tile offsets", (long long)io.y_cstride);
    a.n_cols = (int32_t)p.n_cols;
    if (L.transposed) {
        a.stride = 1; a.dil = -1; a.pad = 0;
        a.y_tstride = L.stride; a.y_toff = -L.pad;
        a.n_phase = L.n_phase;   // 1 in sub-pixel form
    } else {
        a.stride = L.stride; a.dil = L.dil; a.pad = L.pad;
        a.y_tstride = 1; a.y_toff = 0;
        a.n_phase = 1;
    }
    a.xneg = a.dil < 0 ? (L.Ktaps - 1) * p.ad : 0;
    static const bool no_xr = env_flag("NC_NO_XR");
    if (no_xr) a.epi |= EPI_NO_XR;
}

// XV (round 5): vectorised window staging of the two-tap sub-pixel instances and of k = 7 (the kernel's XV note) -- plain input, rows
// and window start on 16-byte boundaries (xneg is raised by up to 3 slots for that: the window still fits its 320-slot pitch), whole
// float4s (k = 7: float2s; see xv_input_ok for what the row alignment is worth there)
static ConvForm xv_form(const ConvLayer& L, const ConvIO& io) {
    return L.sub_stride ? (L.sub_shift ? F_XV_SUB : F_XV_SUBG) : (io.fuse_k1 ? F_XV_FUSED : F_XV);
}
static void plan_xv(ConvPlan& p, const ConvLayer& L, const ConvIO& io) {
    static const bool no_xv = env_flag("NC_NO_XV");
    static const bool no_xr = env_flag("NC_NO_XR");
    static const bool no_xv_k7 = env_flag("NC_NO_XV_K7");
    static const int64_t xv_k7_min = env_int("NC_XV_K7_MIN_COLS", 0);
    const TileCfg& c = p.c;
    const bool xv_k7 = !no_xv_k7 && p.n_cols >= xv_k7_min;
    const bool two_tap = xv_two_tap_layer(L, io) && c.K == 2 && c.CB == 16;
    const bool k7 = xv_k7 && !L.transposed && !L.sub_stride && c.K == 7 && c.CB == 8 && L.stride == 1 && !p.fused_wide;   // (the fused units included)
    const int vw = two_tap ? 4 : 2;   // floats per staged word
    if (no_xv || no_xr || !(two_tap || k7) || c.TN != 2 || c.NW != 4 || c.TM < 2 || c.TM > 4 || p.narrow || p.flat || p.dist || p.slim ||
        p.sx != 1 || L.Cin % c.CB != 0 || !xv_input_ok(io, vw))
        return;
    const int extra = (vw - (p.a.pad + p.a.xneg) % vw) % vw;
    if (p.window(c.BN()) + extra > 320 || !conv_instance(xv_form(L, io), c.K, c.TM, c.TN).fn) return;
    p.xv = true;
    p.xv_extra = extra;
    p.a.xneg += extra;
    p.a.epi |= EPI_XVEC;
}

// Window geometry (the kernel's staging notes), the tile map and the LDS the tile needs.
static void plan_window_and_lds(ConvPlan& p, const ConvLayer& L, const ConvIO& io, int B) {
    ConvArgs& a = p.a;
    const int NW = p.c.NW, BM = p.c.BM(), BN = p.c.BN(), CB = p.c.CB, KB = p.c.KB(), sx = p.sx;
    a.xw = p.window(BN, p.flat ? (p.flat_S - 1) * p.flat_hc : 0) + p.xv_extra;
    a.nchunk = (a.xw + 63) / 64;
    a.xwp = (a.nchunk * 64 + sx - 1) / sx;   // rows are padded to whole 64-slot chunks: every staging store is in-bounds
    a.xrow = sx == 1 ? a.nchunk * 64 : sx * a.xwp;
    a.n_co_tiles = row_tiles(L, p.c);
    a.Bc = B; a.flat = 0; a.flat_px = a.flat_pc = 0x1fffffff; a.flat_hc = 0;
    if (p.flat) {   // one column axis over all clips: B = 1 in the tile map
        a.flat = 1; a.flat_pc = (int32_t)p.flat_pitch; a.flat_hc = p.flat_hc; a.flat_px = (int32_t)(p.flat_pitch + p.flat_hc) * sx;
        a.B = 1;
    }
    a.n_t_tiles = (int32_t)(p.flat ? p.col_tiles_of(B, BN) : col_tiles(1, p.n_cols, BN, false));
    a.n_cb = (L.Cin + CB - 1) / CB;
    a.n_items = CB * a.nchunk;
    if (!p.window_fits(a.xw, NW))
        fail(NC_EUNSUPPORTED, "conv K=%d stride=%d dil=%d: input window of %d words per channel exceeds the staging registers",
             L.K, L.stride, L.dil, a.xw);
    a.xbuf = (((NW * p.nx - 1) / a.nchunk + 1) * a.xrow + 3) & ~3;   // items past n_items land in pad rows
    a.chunk_magic = magic_div(a.nchunk, NW * p.nx + NW);
    a.stride_magic = magic_div(sx, a.nchunk * 64 + 64);
    for (int k = 0; k < 16; ++k) {
        const int q = k * a.dil + a.xneg;
        a.tapoff[k] = (k < L.Ktaps) ? (sx == 1 ? q : (q % sx) * a.xwp + q / sx) : 0;
    }
    size_t lds_f = 2 * (size_t)KB * BM + 2 * (size_t)a.xbuf + ((io.alpha_in || (p.in_mode & 1)) ? 2 * (size_t)a.n_cb * CB * (io.x2 ? 2 : 1) : 0);
    if (io.fuse_k1) lds_f = std::max(lds_f, p.fused_wide ? (size_t)2 * BM * 32 : (size_t)BM * BM);   // the 1x1 weights reuse the tile buffers
    a.ep_off = (int32_t)lds_f;
    p.lds = sizeof(float) * (lds_f + 6 * (size_t)BM);
}

// The instance family of the plan, in the order of precedence: fused, then XV, then distributed, then two-input, then sub-pixel, then
// narrow, then slim, then plain.  A family without an instance for the plan's tile is an error, never another family.
static void plan_instance(ConvPlan& p, const ConvLayer& L, const ConvIO& io) {
    const TileCfg& c = p.c;
    ConvForm form = F_PLAIN;
    if (io.fuse_k1) {
        if (!can_fuse_res_unit(L, *io.fuse_k1) || !io.alpha_out || !io.res || io.epi != 0)
            fail(NC_ESTATE, "internal: residual unit is not fusable");
        p.a.w2 = io.fuse_k1->w_fused.as<float>();
        p.a.bias2 = io.fuse_k1->bias.as<float>();
        p.a.alpha_out2 = io.alpha_out2;
        form = p.fused_wide ? F_FUSEDW : F_FUSED;
        if (!conv_instance(form, c.K, c.TM, c.TN).fn) fail(NC_EUNSUPPORTED, "no fused residual-unit kernel for TM=%d TN=%d", c.TM, c.TN);
        if (p.xv) form = xv_form(L, io);
    } else if (p.xv) form = xv_form(L, io);
    else if (p.dist) form = dist_form(L);
    else if (io.x2) form = in2_form(L);
    else if (subg_layer(L)) form = F_SUBG;
    else if (L.sub_shift) form = p.narrow ? F_SUB_NARROW : F_SUB;
    else if (p.narrow) form = F_NARROW;
    else if (p.slim) form = F_SLIM;
    p.fn = conv_instance(form, c.K, c.TM, c.TN).fn;
    p.form = conv_form_name[form];
    if (p.fn) return;
    if (form == F_IN2 || form == F_IN2_SUB) fail(NC_EUNSUPPORTED, "no two-input conv kernel for K=%d TM=%d TN=%d", c.K, c.TM, c.TN);
    if (form == F_SUBG) fail(NC_EUNSUPPORTED, "no sub-pixel conv kernel for K=%d TM=%d TN=%d (stride %d)", c.K, c.TM, c.TN, L.sub_stride);
    if (form == F_SUB || form == F_SUB_NARROW) fail(NC_EUNSUPPORTED, "no sub-pixel conv kernel for K=%d TM=%d TN=%d", c.K, c.TM, c.TN);
    fail(NC_EUNSUPPORTED, "no conv kernel for TM=%d TN=%d K=%d", c.TM, c.TN, c.K);
}

static void plan_conv_template(ConvPlan& p, const ConvLayer& L, const ConvIO& io, int B) {
    p.in_mode = in_mode_of(io);
    p.sx = L.transposed ? 1 : L.stride;
    p.ad = L.transposed ? 1 : L.dil;
    p.Tout = L.out_len(io.Tin);
    p.n_cols = L.transposed ? io.Tin + L.Ktaps - 1 : p.Tout;
    TileChoice tsel = plan_row_tile(p, L, io, B);
    p.c = tsel.cfg;
    p.nx = plain_geometry(p.c.K).nx;
    plan_column_tile(p);
    plan_narrow(p, L, io);
    plan_flat(p, tsel, L, io, B);
    plan_tn_rounds(p, L, io, B);
    p.fused_wide = io.fuse_k1 && p.c.TM > 4;   // C = 192 / 256 residual unit: whole-channel tile, 128 columns, 4-channel blocks
    if (p.fused_wide) {
        const ConvInstance w = conv_instance(F_FUSEDW, p.c.K, p.c.TM, 1);
        p.c.TN = 1; p.c.CB = w.CB; p.nx = w.nx;
    }
    plan_slim(p, L, io);
    plan_dist(p, L, io, B);
    plan_args(p, tsel, L, io, B);
    plan_xv(p, L, io);
    plan_window_and_lds(p, L, io, B);
    plan_instance(p, L, io);
    if (p.lds > 160 * 1024) fail(NC_EUNSUPPORTED, "conv tile needs %zu B of LDS", p.lds);
    p.a.co_group = pick_co_group(p.a.n_co_tiles, 4.0 * B * L.Cin * (double)io.Tin, 4.0 * L.Cin * (double)L.rows() * L.Ktaps,
                                 (double)p.a.B * p.a.n_t_tiles);
    p.grid = (int64_t)p.a.n_phase * p.a.n_co_tiles * p.a.B * p.a.n_t_tiles;
    p.threads = 64 * p.c.NW;
}

// ---- the template: launch ----------------------------------------------------------------------------------------------------
#ifdef NC_CONV_TRACE
// diagnostic builds: NC_CONV_TRACE_FILE=<path> + NC_CONV_TRACE_SEL="K,Cin,dil" picks the first matching launch (see the kernel's NC_STAMP)
static bool trace_begin(ConvPlan& p, const ConvLayer& L, const ConvIO& io, DevBuf& trace_buf, hipStream_t stream) {
    static const char* trace_file = env_str("NC_CONV_TRACE_FILE");
    static bool traced = false;
    if (!trace_file || traced || io.x2) return false;
    int tk = 7, tc = 384, td = 1;
    if (const char* sel = env_str("NC_CONV_TRACE_SEL")) std::sscanf(sel, "%d,%d,%d", &tk, &tc, &td);
    if (p.c.K != tk || L.Cin != tc || !(L.dil == td || L.transposed) || p.a.n_cb < 16) return false;
    trace_buf.reserve((size_t)16 * 8 * 8 * 8 * 8);
    NC_HIP(hipMemsetAsync(trace_buf.p, 0, (size_t)16 * 8 * 8 * 8 * 8, stream));
    p.a.x2 = trace_buf.as<float>();
    return traced = true;
}
static void trace_end(const ConvPlan& p, DevBuf& trace_buf, hipStream_t stream) {
    std::vector<unsigned long long> hb((size_t)16 * 8 * 8 * 8);
    NC_HIP(hipStreamSynchronize(stream));
    NC_HIP(hipMemcpy(hb.data(), trace_buf.p, hb.size() * 8, hipMemcpyDeviceToHost));
    if (FILE* f = std::fopen(env_str("NC_CONV_TRACE_FILE"), "wb")) {
        const int hdr[8] = {16, p.c.NW, 8, 8, p.c.TM, p.c.TN, p.c.K, (p.a.epi & EPI_XVEC) ? 1 : 0};
        std::fwrite(hdr, sizeof(int), 8, f);
        std::fwrite(hb.data(), 8, hb.size(), f);
        std::fclose(f);
    }
    trace_buf.release();
}
#endif

// NC_LAUNCH_LOG=<path>: one "conv_mfma" line per conv-template launch (class, threads, shape) in launch order.  The template serves several
// kernel classes under one kernel name; tools/pmc_classes.py zips this log with the rocprofv3 counter rows of the same
// kernel name (dispatch order) to attribute HBM traffic / matrix-core busy cycles to exactly the launches a class counts.
// Then the "conv_plan" line of the launch with the plan's decisions: TM TN NW CB flat narrow slim dist xv co_group n_co_tiles
// n_t_tiles n_cb xw xneg.
static void log_plan(const ConvPlan& p, const ConvLayer& L, const ConvIO& io, hipStream_t stream) {
    FILE* lf = launch_log();
    if (!lf) return;
    std::fprintf(lf, "conv_mfma %d %lld %d %d %d %lld %d\n", L.kclass, (long long)p.grid * p.threads, L.Cin, L.Cout, L.K,
                 (long long)io.Tin, io.fuse_k1 ? 1 : 0);
    log_form(lf, p.form, (const void*)p.fn, stream, p.grid, p.threads, p.lds);
    const ConvArgs& a = p.a;
    std::fprintf(lf, " %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", p.c.TM, p.c.TN, p.c.NW, p.c.CB, p.flat, p.narrow, p.slim, p.dist, p.xv,
                 a.co_group, a.n_co_tiles, a.n_t_tiles, a.n_cb, a.xw, a.xneg);
    std::fflush(lf);
}

void launch_conv(const ConvLayer& L, const ConvIO& io, int B, hipStream_t stream, Profiler* prof) {
    if (in_mode_of(io) && (io.alpha_in || io.fuse_k1)) fail(NC_ESTATE, "internal: the Encodec input mode does not combine with Snake / fused units");
    if (io.x2 && (!conv_in2_available(L) || (io.in_stats != nullptr) != (io.in_stats2 != nullptr)))
        fail(NC_ESTATE, "internal: no two-input kernel for this layer");
    if (io.gn_part && !conv_gn_fusable(L, io, B)) fail(NC_ESTATE, "internal: this launch cannot emit GroupNorm block sums");
    if (launch_skinny(L, io, B, stream, prof)) return log_special("skinny");
    if (launch_thin_inm(L, io, B, stream, prof)) return log_special("thin_inm");
    if (launch_thin(L, io, B, stream, prof)) return log_special("thin");
    if (launch_stem(L, io, B, stream, prof)) return log_special("stem");
    if (launch_small(L, io, B, stream, prof)) return log_special("small");
    if (launch_conv1x1(L, io, B, stream, prof)) return;
    if (launch_conv3_stream(L, io, B, stream, prof)) return;
    ConvPlan p;
    plan_conv_template(p, L, io, B);
    ensure_dynamic_lds((const void*)p.fn, 160 * 1024);
    if (p.grid <= 0) return;
#ifdef NC_CONV_TRACE
    DevBuf trace_buf;
    const bool trace_now = trace_begin(p, L, io, trace_buf, stream);
#endif
    {
        ProfScope ps(prof, stream, L.kclass, L.flops(B, io.Tin) + (io.fuse_k1 ? io.fuse_k1->flops(B, io.Tin) : 0.0),
                     conv_bytes(L, B, (double)io.Tin, (double)p.Tout));
        hipLaunchKernelGGL(p.fn, dim3((unsigned)p.grid), dim3(p.threads), p.lds, stream, p.a);
        NC_HIP(hipGetLastError());
    }
#ifdef NC_CONV_TRACE
    if (trace_now) trace_end(p, trace_buf, stream);
#endif
    log_plan(p, L, io, stream);
}

}  // namespace nc
