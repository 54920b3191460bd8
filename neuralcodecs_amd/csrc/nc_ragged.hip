// Ragged batches: DAC / SNAC Encode and Decode of B clips of unequal lengths in one call (include/nc_mi355x.h, "ragged batches").
//
// Planner.  With the halos of the direction (as make_plan of nc_chunk.hip assigns them), a kept width C and W = C + halo_l + halo_r:
//   a clip of F >= W frames is covered by n = 1 + ceil((F - W) / C) windows of exactly W frames at w0_j = min(j * C, F - W).  Window 0 is
//   left-aligned to the clip and keeps [0, C + halo_l); window j keeps [j * C + halo_l, (j + 1) * C + halo_l) = [w0 + halo_l, w0 + W -
//   halo_r); the last is right-aligned (w0 = F - W <= (n - 1) * C) and keeps from where window n - 2 stopped, (n - 1) * C + halo_l >= w0 +
//   halo_l, to F.  So every frame is kept once, every kept frame is halo_l / halo_r away from an interior window edge, and both outer edges
//   of a clip are window edges that are true clip edges.  Clips of F < W frames are one window of width F each; equal F form a group.
// Why it is exact: what nc_chunk.hip rests on (a window edge that is a clip edge gets the layers' own zero padding; an interior edge is
// wrong only inside the halo; every conv instance computes a column from the same operands in the same order wherever the column sits and
// whichever row of the batch it is in), plus one thing of its own: the samples behind a clip's end inside its last window are written as
// +0.0f, which is the value the layers' right zero-pad (DAC's pad to the hop, SNAC's to hop * align) reads there.
// Rows of one width from different clips then go through the EXISTING launch sequences as one uniform batch; no convolution changes.
//
// Kernels.  One table-driven copy per tensor and launch batch instead of one pitched copy per window: a descriptor is a run of n elements
// from src to dst followed by `fill` zeros.  The host writes all tables of a call into pinned memory and copies them once, asynchronously,
// on the handle's stream.  The copy is concat_copy (nc_copy.h), the launch loop over grid.y for_grid_y (nc_pool.h).
#include <algorithm>
#include <cstring>
#include <map>

#include "nc_copy.h"
#include "nc_guard.h"
#include "nc_pool.h"
#include "nc_ragged.h"

namespace nc {

namespace {

// ---- kernels ---------------------------------------------------------------------------------------------------------------------
// Memory-bound, no LDS, no atomics.  blockIdx.y = descriptor, blockIdx.x strides over its run, which concat_copy (nc_copy.h) stores: a
// run of n source elements followed by `fill` zeros is the concatenation of one piece.
template <class T>
__device__ __forceinline__ void ragged_copy_body(const RgSeg* __restrict__ segs, const T* __restrict__ src, T* __restrict__ dst) {
    const RgSeg g = segs[blockIdx.y];
    concat_copy<T>(src + g.src, g.n, nullptr, 0, 0, dst + g.dst, g.n + g.fill);
}

// packed PCM (or SNAC noise) -> dense window rows, zero-filled behind a clip's end
__global__ __launch_bounds__(256) void ragged_gather_f32(const RgSeg* __restrict__ segs, const float* __restrict__ src, float* __restrict__ dst) {
    ragged_copy_body<float>(segs, src, dst);
}
// packed codes -> [N_w, rows, W] window codes (SNAC: every level at its own rate)
__global__ __launch_bounds__(256) void ragged_gather_i64(const RgSeg* __restrict__ segs, const int64_t* __restrict__ src, int64_t* __restrict__ dst) {
    ragged_copy_body<int64_t>(segs, src, dst);
}
// kept columns of the window outputs -> packed destinations
__global__ __launch_bounds__(256) void ragged_scatter_f32(const RgSeg* __restrict__ segs, const float* __restrict__ src, float* __restrict__ dst) {
    ragged_copy_body<float>(segs, src, dst);
}
__global__ __launch_bounds__(256) void ragged_scatter_i64(const RgSeg* __restrict__ segs, const int64_t* __restrict__ src, int64_t* __restrict__ dst) {
    ragged_copy_body<int64_t>(segs, src, dst);
}

// ---- planner ---------------------------------------------------------------------------------------------------------------------
// the best measured pairs of profiles/ragged_bench.json
constexpr int64_t kDefaultKeptDac = 128, kDefaultKeptSnac = 256;
constexpr int32_t kDefaultMaxWindows = kRaggedDefaultMaxWindows;

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

struct RgRow { int32_t clip; int64_t w0, k0, n; };            // frames [w0, w0 + W) of the clip; kept [w0 + k0, w0 + k0 + n)
struct RgBatch { int64_t W; int64_t first, count; };           // rows [first, first + count) of width W
struct RgPlan {
    int64_t W = 0, C = 0, hl = 0, hr = 0;
    int32_t maxw = 0;
    std::vector<RgRow> rows;
    std::vector<RgBatch> batches;
    int64_t n_windows = 0, n_window_batches = 0, n_groups = 0, total_frames = 0;
};

RgPlan make_ragged_plan(int B, const int64_t* frames, int64_t hl, int64_t hr, int64_t align, int64_t kept, int64_t default_kept, int32_t maxw) {
    if (B <= 0 || !frames) fail(NC_EINVAL, "B must be positive and frames must not be null");
    if (kept < 0 || maxw < 0) fail(NC_EINVAL, "kept_frames and max_windows must not be negative (0 = default)");
    RgPlan P;
    P.C = ceil_div(kept > 0 ? kept : default_kept, align) * align;
    P.maxw = maxw > 0 ? maxw : kDefaultMaxWindows;
    P.hl = hl; P.hr = hr;
    P.W = P.C + hl + hr;
    std::map<int64_t, std::vector<int32_t>> groups;
    for (int b = 0; b < B; ++b) {
        const int64_t F = frames[b];
        if (F <= 0) fail(NC_EINVAL, "clip %d: frame count must be positive", b);
        if (F > (int64_t)1 << 40) fail(NC_EINVAL, "clip %d: clip too long", b);
        if (F % align != 0) fail(NC_EINVAL, "clip %d: frame count %lld is not a multiple of %lld", b, (long long)F, (long long)align);
        P.total_frames += F;
        if (F < P.W) { groups[F].push_back(b); continue; }
        const int64_t n = 1 + ceil_div(F - P.W, P.C);
        int64_t kept_to = 0;
        for (int64_t j = 0; j < n; ++j) {
            const int64_t w0 = std::min(j * P.C, F - P.W);
            const int64_t k1 = j + 1 == n ? F : w0 + P.W - hr;
            P.rows.push_back({b, w0, kept_to - w0, k1 - kept_to});
            kept_to = k1;
        }
        P.n_windows += n;
    }
    for (int64_t r = 0; r < P.n_windows; r += P.maxw) P.batches.push_back({P.W, r, std::min<int64_t>(P.maxw, P.n_windows - r)});
    P.n_window_batches = (int64_t)P.batches.size();
    P.n_groups = (int64_t)groups.size();
    for (const auto& g : groups) {
        const int64_t first = (int64_t)P.rows.size(), n = (int64_t)g.second.size();
        for (int32_t b : g.second) P.rows.push_back({b, 0, 0, g.first});
        for (int64_t r = 0; r < n; r += P.maxw) P.batches.push_back({g.first, first + r, std::min<int64_t>(P.maxw, n - r)});
    }
    return P;
}

void halos_of(const nc_halo& h, bool decode, int64_t& hl, int64_t& hr) {   // as make_plan (nc_chunk.hip)
    hl = decode ? h.dec_right : h.enc_right;
    hr = decode ? h.dec_left : h.enc_left;
}

void report(const RgPlan& P, int64_t arena, int64_t total_codes, int64_t total_samples, nc_ragged_plan* out, nc_ragged_window* windows, int64_t cap) {
    out->window_frames = P.W; out->kept_frames = P.C; out->halo_left = P.hl; out->halo_right = P.hr;
    out->n_windows = P.n_windows; out->n_window_batches = P.n_window_batches; out->n_exact_groups = P.n_groups;
    out->n_rows = (int64_t)P.rows.size(); out->n_batches = (int64_t)P.batches.size();
    out->arena_bytes = arena; out->total_frames = P.total_frames; out->total_codes = total_codes; out->total_samples = total_samples;
    if (!windows) return;
    for (size_t bi = 0; bi < P.batches.size(); ++bi)
        for (int64_t r = P.batches[bi].first; r < P.batches[bi].first + P.batches[bi].count && r < cap; ++r) {
            const RgRow& w = P.rows[(size_t)r];
            windows[r] = {w.clip, (int32_t)bi, w.w0, P.batches[bi].W, w.w0 + w.k0, w.n};
        }
}

int64_t dac_decoded_len(const nc_dac_config& c, int64_t fr) {   // DacModel::decoded_len on the config
    int64_t L = fr;
    for (int i = 0; i < c.n_decoder_rates; ++i) { const int64_t s = c.decoder_rates[i]; L = (L - 1) * s - 2 * ((s + 1) / 2) + 2 * s; }
    return L;
}

void dac_plan_report(const nc_dac_config& c, bool decode, int B, const int64_t* frames, int64_t kept, int32_t maxw, nc_ragged_plan* out,
                     nc_ragged_window* windows, int64_t cap) {
    if (!out) fail(NC_EINVAL, "out must not be null");
    nc_halo h{};
    if (nc_dac_halo(&c, &h) != NC_OK) fail(NC_EINVAL, "%s", get_last_error());
    int64_t hl, hr;
    halos_of(h, decode, hl, hr);
    const RgPlan P = make_ragged_plan(B, frames, hl, hr, h.align, kept, kDefaultKeptDac, maxw);
    int64_t samples = 0;
    for (int b = 0; b < B; ++b) samples += dac_decoded_len(c, frames[b]);
    report(P, DacModel::arena_bytes(c, decode ? CK_DECODE : CK_ENCODE, P.maxw, P.W), (int64_t)c.n_codebooks * P.total_frames, samples, out, windows, cap);
}

void snac_plan_report(const nc_snac_config& c, bool decode, int B, const int64_t* frames, int64_t kept, int32_t maxw, nc_ragged_plan* out,
                      nc_ragged_window* windows, int64_t cap) {
    if (!out) fail(NC_EINVAL, "out must not be null");
    nc_halo h{};
    if (nc_snac_halo(&c, &h) != NC_OK) fail(NC_EINVAL, "%s", get_last_error());
    int64_t hl, hr;
    halos_of(h, decode, hl, hr);
    const RgPlan P = make_ragged_plan(B, frames, hl, hr, h.align, kept, kDefaultKeptSnac, maxw);
    int64_t codes = 0, samples = 0;
    for (int b = 0; b < B; ++b) {
        for (int i = 0; i < c.n_vq_strides; ++i) codes += frames[b] / c.vq_strides[i];
        int64_t L = frames[b];
        for (int i = 0; i < c.n_decoder_rates; ++i) L = SnacModel::up_len(L, c.decoder_rates[i]);
        samples += L;
    }
    report(P, SnacModel::arena_bytes(c, decode ? CK_DECODE : CK_ENCODE, P.maxw, P.W), codes, samples, out, windows, cap);
}

// ---- the tables of one call (nc_ragged.h) ------------------------------------------------------------------------------------------
using Tables = RgTables;

const char* upload(Codec& m, const Tables& t) {
    Codec::RaggedTables& r = m.rg_tab;
    const size_t seg_bytes = t.segs.size() * sizeof(RgSeg), bytes = seg_bytes + t.extra.size();
    if (!bytes) return nullptr;
    if (!r.ev) NC_HIP(hipEventCreateWithFlags(&r.ev, hipEventDisableTiming));
    if (r.ev_used) NC_HIP(hipEventSynchronize(r.ev));   // the previous call's copy has read the pinned image
    if (bytes > r.pin_cap) {
        if (r.pin) NC_HIP(hipHostFree(r.pin));
        r.pin = nullptr; r.pin_cap = 0;
        const size_t want = (bytes + 65535) & ~(size_t)65535;
        NC_HIP(hipHostMalloc(&r.pin, want, hipHostMallocDefault));
        r.pin_cap = want;
    }
    if (seg_bytes) std::memcpy(r.pin, t.segs.data(), seg_bytes);
    if (!t.extra.empty()) std::memcpy(static_cast<char*>(r.pin) + seg_bytes, t.extra.data(), t.extra.size());
    r.dev.reserve(bytes);
    NC_HIP(hipMemcpyAsync(r.dev.p, r.pin, bytes, hipMemcpyHostToDevice, m.stream));
    NC_HIP(hipEventRecord(r.ev, m.stream));
    r.ev_used = true;
    return t.extra.empty() ? nullptr : r.dev.as<char>() + seg_bytes;
}

template <class T>
void launch(Codec& m, const Tables& t, size_t which, void (*kernel)(const RgSeg*, const T*, T*), const T* src, T* dst) {
    const Tables::Launch& L = t.launches[which];
    const unsigned gx = copy_grid_x(L.longest, sizeof(T));
    for_grid_y(L.count, [&](size_t done, size_t cnt) {
        double bytes = 0;
        if (m.prof.on)
            for (size_t i = 0; i < cnt; ++i) { const RgSeg& g = t.segs[L.first + done + i]; bytes += (double)(2 * g.n + g.fill) * sizeof(T); }
        ProfScope ps(&m.prof, m.stream, NC_KC_ELEM, 0.0, bytes);
        hipLaunchKernelGGL(kernel, dim3(gx, (unsigned)cnt), dim3(256), 0, m.stream, m.rg_tab.dev.as<RgSeg>() + L.first + done, src, dst);
        NC_HIP(hipGetLastError());
    });
}

std::vector<int64_t> prefix(int B, const std::vector<int64_t>& per_clip) {
    std::vector<int64_t> off((size_t)B + 1, 0);
    for (int b = 0; b < B; ++b) off[(size_t)b + 1] = off[(size_t)b] + per_clip[(size_t)b];
    return off;
}

// Packed tensors of a host-pointer call are staged whole: `in` (and the noise) uploaded before the first launch, `out` downloaded behind
// the last.  A device-pointer call works on the caller's arrays.
template <class T>
const T* stage_in(Codec& m, bool host, DevBuf& buf, const T* p, int64_t n) {
    if (!host) return p;
    buf.reserve((size_t)n * sizeof(T));
    NC_HIP(hipMemcpyAsync(buf.p, p, (size_t)n * sizeof(T), hipMemcpyHostToDevice, m.stream));
    return buf.as<T>();
}
template <class T>
T* stage_out(Codec& m, bool host, T* p, int64_t n) {
    if (!host) return p;
    m.rg_out.reserve((size_t)n * sizeof(T));
    return m.rg_out.as<T>();
}
template <class T>
void finish_out(Codec& m, bool host, T* p, int64_t n) {
    if (host) NC_HIP(hipMemcpyAsync(p, m.rg_out.p, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, m.stream));
}

void check_batch(int B, const int64_t* per_clip, const void* in, const void* out, const char* what) {
    if (!in || !out || !per_clip) fail(NC_EINVAL, "%s: null pointer", what);
    if (B <= 0) fail(NC_EINVAL, "%s: B must be positive", what);
    for (int b = 0; b < B; ++b)
        if (per_clip[b] <= 0) fail(NC_EINVAL, "%s: clip %d has length %lld", what, b, (long long)per_clip[b]);
}

RgPlan plan_of(const Codec& m, const nc_halo& h, bool decode, int B, const int64_t* frames, int64_t default_kept) {
    int64_t hl, hr;
    halos_of(h, decode, hl, hr);
    return make_ragged_plan(B, frames, hl, hr, h.align, m.ragged_kept, default_kept, m.ragged_max_windows);
}

// ======================================================================================================================== DAC
void dac_encode_ragged(DacModel& m, bool host, const float* pcm, int B, const int64_t* lengths, int sample_rate, int n_q, int64_t* codes) {
    check_batch(B, lengths, pcm, codes, "nc_dac_encode_ragged");
    if (!m.loaded) fail(NC_ESTATE, "weights not loaded (call nc_codec_load_weights first)");
    if (sample_rate != 0 && sample_rate != m.cfg.sample_rate)
        fail(NC_EINVAL, "Input audio sample rate %dHz does not match model sample rate %dHz", sample_rate, m.cfg.sample_rate);
    const int nq = (n_q <= 0 || n_q > m.cfg.n_codebooks) ? m.cfg.n_codebooks : n_q;
    const int64_t hop = m.hop;
    std::vector<int64_t> T(lengths, lengths + B), F((size_t)B), NC((size_t)B);
    for (int b = 0; b < B; ++b) {
        if (T[(size_t)b] > (int64_t)1 << 30) fail(NC_EINVAL, "clip too long");
        F[(size_t)b] = m.frames(T[(size_t)b]);
        NC[(size_t)b] = nq * F[(size_t)b];
    }
    nc_halo h{};
    if (nc_dac_halo(&m.cfg, &h) != NC_OK) fail(NC_EINVAL, "%s", get_last_error());
    const RgPlan P = plan_of(m, h, false, B, F.data(), kDefaultKeptDac);
    const std::vector<int64_t> in_off = prefix(B, T), out_off = prefix(B, NC);
    Tables t;
    for (const RgBatch& bt : P.batches) {
        const int64_t Tw = bt.W * hop;
        t.begin(in_off.back(), bt.count * Tw);
        for (int64_t r = 0; r < bt.count; ++r) {
            const RgRow& w = P.rows[(size_t)(bt.first + r)];
            const int64_t n = std::min(T[(size_t)w.clip] - w.w0 * hop, Tw);
            t.add(in_off[(size_t)w.clip] + w.w0 * hop, r * Tw, n, Tw - n);
        }
        t.end();
        t.begin(bt.count * nq * bt.W, out_off.back());
        for (int64_t r = 0; r < bt.count; ++r) {
            const RgRow& w = P.rows[(size_t)(bt.first + r)];
            for (int q = 0; q < nq; ++q) t.add((r * nq + q) * bt.W + w.k0, out_off[(size_t)w.clip] + q * F[(size_t)w.clip] + w.w0 + w.k0, w.n);
        }
        t.end();
    }
    m.use_device();
    const float* src = stage_in(m, host, m.rg_in, pcm, in_off.back());
    int64_t* dst = stage_out(m, host, codes, out_off.back());
    upload(m, t);
    size_t li = 0;
    for (const RgBatch& bt : P.batches) {
        const int64_t Tw = bt.W * hop;
        m.ck_in.reserve((size_t)(bt.count * Tw) * 4);
        m.ck_codes.reserve((size_t)(bt.count * nq * bt.W) * 8);
        launch<float>(m, t, li++, ragged_gather_f32, src, m.ck_in.as<float>());
        m.encode_dev(m.ck_in.as<float>(), (int)bt.count, Tw, sample_rate, n_q, m.ck_codes.as<int64_t>(), nullptr, nullptr);
        launch<int64_t>(m, t, li++, ragged_scatter_i64, m.ck_codes.as<int64_t>(), dst);
    }
    finish_out(m, host, codes, out_off.back());
}

void dac_decode_ragged(DacModel& m, bool host, const int64_t* codes, int B, const int64_t* frames, int n_q, float* pcm) {
    check_batch(B, frames, codes, pcm, "nc_dac_decode_codes_ragged");
    if (!m.loaded) fail(NC_ESTATE, "weights not loaded (call nc_codec_load_weights first)");
    if (n_q <= 0 || n_q > m.cfg.n_codebooks) fail(NC_EINVAL, "bad codes shape: n_q = %d", n_q);
    nc_halo h{};
    if (nc_dac_halo(&m.cfg, &h) != NC_OK) fail(NC_EINVAL, "%s", get_last_error());
    const RgPlan P = plan_of(m, h, true, B, frames, kDefaultKeptDac);
    int64_t H = 1;   // output samples per frame: a window's samples sit at frame * H exactly (DacModel::decode)
    for (int i = 0; i < m.cfg.n_decoder_rates; ++i) H *= m.cfg.decoder_rates[i];
    std::vector<int64_t> NC((size_t)B), L((size_t)B);
    for (int b = 0; b < B; ++b) {
        NC[(size_t)b] = n_q * frames[b];
        L[(size_t)b] = m.decoded_len(frames[b]);
        if (L[(size_t)b] <= 0) fail(NC_EINVAL, "clip %d: %lld frames decode to nothing", b, (long long)frames[b]);
    }
    const std::vector<int64_t> in_off = prefix(B, NC), out_off = prefix(B, L);
    Tables t;
    for (const RgBatch& bt : P.batches) {
        const int64_t Lw = m.decoded_len(bt.W);
        t.begin(in_off.back(), bt.count * n_q * bt.W);
        for (int64_t r = 0; r < bt.count; ++r) {
            const RgRow& w = P.rows[(size_t)(bt.first + r)];
            for (int q = 0; q < n_q; ++q) t.add(in_off[(size_t)w.clip] + q * frames[w.clip] + w.w0, (r * n_q + q) * bt.W, bt.W);
        }
        t.end();
        t.begin(bt.count * Lw, out_off.back());
        for (int64_t r = 0; r < bt.count; ++r) {
            const RgRow& w = P.rows[(size_t)(bt.first + r)];
            const int64_t f0 = w.w0 + w.k0, f1 = f0 + w.n, o0 = f0 * H, o1 = f1 == frames[w.clip] ? L[(size_t)w.clip] : f1 * H;
            if (w.k0 * H + (o1 - o0) > Lw) fail(NC_ESTATE, "internal: decoded window of %lld samples does not cover its kept frames", (long long)Lw);
            t.add(r * Lw + w.k0 * H, out_off[(size_t)w.clip] + o0, std::max<int64_t>(0, o1 - o0));
        }
        t.end();
    }
    m.use_device();
    const int64_t* src = stage_in(m, host, m.rg_in, codes, in_off.back());
    float* dst = stage_out(m, host, pcm, out_off.back());
    upload(m, t);
    size_t li = 0;
    for (const RgBatch& bt : P.batches) {
        const int N = (int)bt.count;
        m.ck_codes.reserve((size_t)(bt.count * n_q * bt.W) * 8);
        m.ck_a.reserve((size_t)(bt.count * m.latent * bt.W) * 4);
        m.ck_out.reserve((size_t)(bt.count * m.decoded_len(bt.W)) * 4);
        launch<int64_t>(m, t, li++, ragged_gather_i64, src, m.ck_codes.as<int64_t>());
        m.from_codes_dev(m.ck_codes.as<int64_t>(), N, n_q, bt.W, m.ck_a.as<float>());
        m.decode_dev(m.ck_a.as<float>(), N, bt.W, m.ck_out.as<float>());
        launch<float>(m, t, li++, ragged_scatter_f32, m.ck_out.as<float>(), dst);
    }
    finish_out(m, host, pcm, out_off.back());
}

// ======================================================================================================================= SNAC
void snac_encode_ragged(SnacModel& m, bool host, const float* pcm, int B, const int64_t* lengths, int64_t* codes) {
    check_batch(B, lengths, pcm, codes, "nc_snac_encode_ragged");
    if (!m.loaded) fail(NC_ESTATE, "weights not loaded (call nc_codec_load_weights first)");
    const int64_t hop = m.hop;
    const int nl = m.cfg.n_vq_strides;
    std::vector<int64_t> T(lengths, lengths + B), F((size_t)B), NC((size_t)B);
    for (int b = 0; b < B; ++b) {
        if (T[(size_t)b] > (int64_t)1 << 30) fail(NC_EINVAL, "B and T must be positive");
        F[(size_t)b] = m.padded_len(T[(size_t)b]) / hop;
        NC[(size_t)b] = m.codes_per_clip(F[(size_t)b]);
    }
    nc_halo h{};
    if (nc_snac_halo(&m.cfg, &h) != NC_OK) fail(NC_EINVAL, "%s", get_last_error());
    const RgPlan P = plan_of(m, h, false, B, F.data(), kDefaultKeptSnac);
    const std::vector<int64_t> in_off = prefix(B, T), out_off = prefix(B, NC);
    Tables t;
    for (const RgBatch& bt : P.batches) {
        const int64_t Tw = bt.W * hop, cw = m.codes_per_clip(bt.W);
        if (m.padded_len(Tw) != Tw) fail(NC_ESTATE, "internal: window of %lld frames is not whole padding units", (long long)bt.W);
        t.begin(in_off.back(), bt.count * Tw);
        for (int64_t r = 0; r < bt.count; ++r) {
            const RgRow& w = P.rows[(size_t)(bt.first + r)];
            const int64_t n = std::max<int64_t>(0, std::min(T[(size_t)w.clip] - w.w0 * hop, Tw));
            t.add(in_off[(size_t)w.clip] + w.w0 * hop, r * Tw, n, Tw - n);
        }
        t.end();
        t.begin(bt.count * cw, out_off.back());
        for (int64_t r = 0; r < bt.count; ++r) {
            const RgRow& w = P.rows[(size_t)(bt.first + r)];
            int64_t os = 0, od = 0;
            for (int i = 0; i < nl; ++i) {   // every level at its own rate (SnacModel::copy_levels)
                const int64_t s = m.cfg.vq_strides[i];
                t.add(r * cw + os + w.k0 / s, out_off[(size_t)w.clip] + od + (w.w0 + w.k0) / s, w.n / s);
                os += bt.W / s; od += F[(size_t)w.clip] / s;
            }
        }
        t.end();
    }
    m.use_device();
    const float* src = stage_in(m, host, m.rg_in, pcm, in_off.back());
    int64_t* dst = stage_out(m, host, codes, out_off.back());
    upload(m, t);
    size_t li = 0;
    for (const RgBatch& bt : P.batches) {
        const int64_t Tw = bt.W * hop;
        m.ck_in.reserve((size_t)(bt.count * Tw) * 4);
        m.ck_codes.reserve((size_t)(bt.count * m.codes_per_clip(bt.W)) * 8);
        launch<float>(m, t, li++, ragged_gather_f32, src, m.ck_in.as<float>());
        m.encode_dev(m.ck_in.as<float>(), (int)bt.count, Tw, m.ck_codes.as<int64_t>(), nullptr, nullptr, true);
        launch<int64_t>(m, t, li++, ragged_scatter_i64, m.ck_codes.as<int64_t>(), dst);
    }
    finish_out(m, host, codes, out_off.back());
}

void snac_decode_ragged(SnacModel& m, bool host, const int64_t* codes, int B, const int64_t* frames, const float* noise, uint64_t seed, float* pcm) {
    check_batch(B, frames, codes, pcm, "nc_snac_decode_ragged");
    if (!m.loaded) fail(NC_ESTATE, "weights not loaded (call nc_codec_load_weights first)");
    const int nl = m.cfg.n_vq_strides, nd = m.cfg.n_decoder_rates;
    const bool with_noise = m.cfg.noise != 0;
    nc_halo h{};
    if (nc_snac_halo(&m.cfg, &h) != NC_OK) fail(NC_EINVAL, "%s", get_last_error());
    const RgPlan P = plan_of(m, h, true, B, frames, kDefaultKeptSnac);   // refuses frame counts that are not whole pooling blocks and attention windows
    std::vector<int64_t> NC((size_t)B), L((size_t)B), NZ((size_t)B);
    for (int b = 0; b < B; ++b) {
        NC[(size_t)b] = m.codes_per_clip(frames[b]);
        L[(size_t)b] = m.decoded_len(frames[b]);
        NZ[(size_t)b] = m.noise_len(1, frames[b]);
    }
    const std::vector<int64_t> in_off = prefix(B, NC), out_off = prefix(B, L), nz_off = prefix(B, NZ);
    Tables t;
    for (const RgBatch& bt : P.batches) {
        const int64_t cw = m.codes_per_clip(bt.W), Lw = m.decoded_len(bt.W);
        t.begin(in_off.back(), bt.count * cw);
        for (int64_t r = 0; r < bt.count; ++r) {
            const RgRow& w = P.rows[(size_t)(bt.first + r)];
            int64_t os = 0, od = 0;
            for (int i = 0; i < nl; ++i) {
                const int64_t s = m.cfg.vq_strides[i];
                t.add(in_off[(size_t)w.clip] + os + w.w0 / s, r * cw + od, bt.W / s);
                os += frames[w.clip] / s; od += bt.W / s;
            }
        }
        t.end();
        if (with_noise) {   // one [N, W * S_i] block per decoder stage, stages end to end (SnacModel::decode_dev)
            t.begin(nz_off.back(), m.noise_len((int)bt.count, bt.W));
            int64_t S = 1, off_w = 0;
            std::vector<int64_t> off_c((size_t)bt.count, 0);
            for (int i = 0; i < nd; ++i) {
                S *= m.cfg.decoder_rates[i];
                for (int64_t r = 0; r < bt.count; ++r) {
                    const RgRow& w = P.rows[(size_t)(bt.first + r)];
                    t.add(nz_off[(size_t)w.clip] + off_c[(size_t)r] + w.w0 * S, off_w + r * bt.W * S, bt.W * S);
                    off_c[(size_t)r] += frames[w.clip] * S;
                }
                off_w += bt.count * bt.W * S;
            }
            t.end();
        }
        const int64_t Hs = Lw / bt.W;   // = hop: every SNAC up-conv maps L -> L * s
        t.begin(bt.count * Lw, out_off.back());
        for (int64_t r = 0; r < bt.count; ++r) {
            const RgRow& w = P.rows[(size_t)(bt.first + r)];
            t.add(r * Lw + w.k0 * Hs, out_off[(size_t)w.clip] + (w.w0 + w.k0) * Hs, w.n * Hs);
        }
        t.end();
    }
    m.use_device();
    const int64_t* src = stage_in(m, host, m.rg_in, codes, in_off.back());
    const float* nz = nullptr;
    if (with_noise && noise) {
        nz = stage_in(m, host, m.rg_noise, noise, nz_off.back());
    } else if (with_noise) {   // clip b exactly as nc_snac_decode(B = 1, seed + b) draws it
        m.rg_noise.reserve((size_t)nz_off.back() * 4);
        for (int b = 0; b < B; ++b) launch_randn(m.rg_noise.as<float>() + nz_off[(size_t)b], NZ[(size_t)b], seed + (uint64_t)b, m.stream);
        nz = m.rg_noise.as<float>();
    }
    float* dst = stage_out(m, host, pcm, out_off.back());
    upload(m, t);
    size_t li = 0;
    for (const RgBatch& bt : P.batches) {
        const int N = (int)bt.count;
        m.ck_codes.reserve((size_t)(bt.count * m.codes_per_clip(bt.W)) * 8);
        m.ck_out.reserve((size_t)(bt.count * m.decoded_len(bt.W)) * 4);
        launch<int64_t>(m, t, li++, ragged_gather_i64, src, m.ck_codes.as<int64_t>());
        if (with_noise) {
            m.ck_noise.reserve((size_t)m.noise_len(N, bt.W) * 4);
            launch<float>(m, t, li++, ragged_gather_f32, nz, m.ck_noise.as<float>());
        }
        m.decode_dev(m.ck_codes.as<int64_t>(), N, bt.W, with_noise ? m.ck_noise.as<float>() : nullptr, seed, m.ck_out.as<float>());
        launch<float>(m, t, li++, ragged_scatter_f32, m.ck_out.as<float>(), dst);
    }
    finish_out(m, host, pcm, out_off.back());
}

// A host-pointer call: on the handle's own stream, complete on return.
template <class F>
void host_call(Codec& m, F&& f) {
    OwnStreamScope own(m);
    f();
    NC_HIP(hipStreamSynchronize(m.stream));
}

}  // namespace

const char* rg_upload(Codec& m, const RgTables& t) { return upload(m, t); }
void rg_copy_f32(Codec& m, const RgTables& t, size_t which, const float* src, float* dst) { launch<float>(m, t, which, ragged_gather_f32, src, dst); }
void rg_copy_i64(Codec& m, const RgTables& t, size_t which, const int64_t* src, int64_t* dst) { launch<int64_t>(m, t, which, ragged_gather_i64, src, dst); }

Codec::RaggedTables::~RaggedTables() {
    if (ev) (void)hipEventDestroy(ev);
    if (pin) (void)hipHostFree(pin);
}

}  // namespace nc

// ================================================================================================ C ABI
using namespace nc;

extern "C" {

nc_status nc_dac_ragged_windows(const nc_dac_config* cfg, int32_t decode, int32_t B, const int64_t* frames, int64_t kept_frames, int32_t max_windows,
                                nc_ragged_plan* out, nc_ragged_window* windows, int64_t cap) {
    return guard([&] {
        if (!cfg) fail(NC_EINVAL, "cfg must not be null");
        dac_plan_report(*cfg, decode != 0, B, frames, kept_frames, max_windows, out, windows, cap);
    });
}

nc_status nc_snac_ragged_windows(const nc_snac_config* cfg, int32_t decode, int32_t B, const int64_t* frames, int64_t kept_frames, int32_t max_windows,
                                 nc_ragged_plan* out, nc_ragged_window* windows, int64_t cap) {
    return guard([&] {
        if (!cfg) fail(NC_EINVAL, "cfg must not be null");
        snac_plan_report(*cfg, decode != 0, B, frames, kept_frames, max_windows, out, windows, cap);
    });
}

nc_status nc_codec_set_ragged_window(nc_codec* h, int64_t kept_frames, int32_t max_windows) {
    return guard([&] {
        Codec& c = codec_of(h);
        if (h->kind == EncodecModel::kKind) fail(NC_EUNSUPPORTED, "Encodec handles are not cut into windows (48 kHz is segmented per second already, the 24 kHz LSTM has unbounded context): their ragged calls pool segments, see nc_encodec_set_ragged_rows");
        if (kept_frames < 0 || max_windows < 0) fail(NC_EINVAL, "kept_frames and max_windows must not be negative (0 = default)");
        c.ragged_kept = kept_frames;
        c.ragged_max_windows = max_windows;
    });
}

nc_status nc_codec_ragged_plan(const nc_codec* h, int32_t decode, int32_t B, const int64_t* frames, nc_ragged_plan* out) {
    return guard([&] {
        Codec& c = codec_of(h);
        if (h->kind == EncodecModel::kKind) fail(NC_EUNSUPPORTED, "Encodec handles have no window plan: see nc_encodec_ragged_rows");
        if (h->kind == DacModel::kKind) dac_plan_report(as<DacModel>(h).cfg, decode != 0, B, frames, c.ragged_kept, c.ragged_max_windows, out, nullptr, 0);
        else snac_plan_report(as<SnacModel>(h).cfg, decode != 0, B, frames, c.ragged_kept, c.ragged_max_windows, out, nullptr, 0);
    });
}

nc_status nc_dac_ragged_query(const nc_codec* h, int32_t B, const int64_t* lengths, int64_t* frames, int64_t* decoded_lens) {
    return guard([&] {
        DacModel& m = as<DacModel>(h);
        if (B <= 0 || !lengths) fail(NC_EINVAL, "B must be positive and lengths must not be null");
        for (int b = 0; b < B; ++b) {
            if (lengths[b] <= 0) fail(NC_EINVAL, "clip %d has length %lld", b, (long long)lengths[b]);
            if (frames) frames[b] = m.frames(lengths[b]);
            if (decoded_lens) decoded_lens[b] = m.decoded_len(m.frames(lengths[b]));
        }
    });
}

nc_status nc_snac_ragged_query(const nc_codec* h, int32_t B, const int64_t* lengths, int64_t* frames, int64_t* codes_per_clip, int64_t* decoded_lens) {
    return guard([&] {
        SnacModel& m = as<SnacModel>(h);
        if (B <= 0 || !lengths) fail(NC_EINVAL, "B must be positive and lengths must not be null");
        for (int b = 0; b < B; ++b) {
            if (lengths[b] <= 0) fail(NC_EINVAL, "clip %d has length %lld", b, (long long)lengths[b]);
            const int64_t F = m.padded_len(lengths[b]) / m.hop;
            if (frames) frames[b] = F;
            if (codes_per_clip) codes_per_clip[b] = m.codes_per_clip(F);
            if (decoded_lens) decoded_lens[b] = m.decoded_len(F);
        }
    });
}

nc_status nc_dac_encode_ragged_dev(nc_codec* h, const float* pcm_packed, int32_t B, const int64_t* lengths, int32_t sample_rate, int32_t n_q,
                                   int64_t* codes_packed) {
    return guard([&] { dac_encode_ragged(as<DacModel>(h), false, pcm_packed, B, lengths, sample_rate, n_q, codes_packed); });
}
nc_status nc_dac_encode_ragged(nc_codec* h, const float* pcm_packed, int32_t B, const int64_t* lengths, int32_t sample_rate, int32_t n_q,
                               int64_t* codes_packed) {
    return guard([&] {
        DacModel& m = as<DacModel>(h);
        check_batch(B, lengths, pcm_packed, codes_packed, "nc_dac_encode_ragged");
        host_call(m, [&] { dac_encode_ragged(m, true, pcm_packed, B, lengths, sample_rate, n_q, codes_packed); });
    });
}
nc_status nc_dac_decode_codes_ragged_dev(nc_codec* h, const int64_t* codes_packed, int32_t B, const int64_t* frames, int32_t n_q, float* pcm_packed) {
    return guard([&] { dac_decode_ragged(as<DacModel>(h), false, codes_packed, B, frames, n_q, pcm_packed); });
}
nc_status nc_dac_decode_codes_ragged(nc_codec* h, const int64_t* codes_packed, int32_t B, const int64_t* frames, int32_t n_q, float* pcm_packed) {
    return guard([&] {
        DacModel& m = as<DacModel>(h);
        check_batch(B, frames, codes_packed, pcm_packed, "nc_dac_decode_codes_ragged");
        host_call(m, [&] { dac_decode_ragged(m, true, codes_packed, B, frames, n_q, pcm_packed); });
    });
}
nc_status nc_snac_encode_ragged_dev(nc_codec* h, const float* pcm_packed, int32_t B, const int64_t* lengths, int64_t* codes_packed) {
    return guard([&] { snac_encode_ragged(as<SnacModel>(h), false, pcm_packed, B, lengths, codes_packed); });
}
nc_status nc_snac_encode_ragged(nc_codec* h, const float* pcm_packed, int32_t B, const int64_t* lengths, int64_t* codes_packed) {
    return guard([&] {
        SnacModel& m = as<SnacModel>(h);
        check_batch(B, lengths, pcm_packed, codes_packed, "nc_snac_encode_ragged");
        host_call(m, [&] { snac_encode_ragged(m, true, pcm_packed, B, lengths, codes_packed); });
    });
}
nc_status nc_snac_decode_ragged_dev(nc_codec* h, const int64_t* codes_packed, int32_t B, const int64_t* frames, const float* noise, uint64_t seed,
                                    float* pcm_packed) {
    return guard([&] { snac_decode_ragged(as<SnacModel>(h), false, codes_packed, B, frames, noise, seed, pcm_packed); });
}
nc_status nc_snac_decode_ragged(nc_codec* h, const int64_t* codes_packed, int32_t B, const int64_t* frames, const float* noise, uint64_t seed,
                                float* pcm_packed) {
    return guard([&] {
        SnacModel& m = as<SnacModel>(h);
        check_batch(B, frames, codes_packed, pcm_packed, "nc_snac_decode_ragged");
        host_call(m, [&] { snac_decode_ragged(m, true, codes_packed, B, frames, noise, seed, pcm_packed); });
    });
}

}  // extern "C"
