// Encodec ragged batches: Encode and Decode of B clips of unequal lengths in one call (include/nc_mi355x.h, "Encodec ragged batches").
//
// Planner.  The reference cuts every clip into segments (Encodec.cs:278-282) and runs EncodeFrame / DecodeFrame on each; a segment depends
// on nothing outside itself -- GroupNorm(1,C), the RMS scale, the LSTM state and the RVQ are all per sample -- which is what
// EncodecModel::for_each_group rests on when it runs a clip's equal-length segments as one batch.  The same holds ACROSS clips: a row is
// one (clip, segment) pair, its key the segment's sample count (Encode) or code-frame count (Decode), and rows of equal key from any clips
// form batches of at most max_rows rows.  Keys run in descending order, the rows of a key segment-major and then by clip, which for equal
// lengths is the uniform call's grouping.  A model without segmentation has one row per clip whose key is the clip's own length: only
// equal-length clips share a batch.
// Why it is exact: every launch of encode_batch / decode_batch computes a row from that row's operands alone, in an order that does not
// depend on the row's index or on the number of rows (the batch invariance tests/test_encodec_gpu.py holds the uniform call to), so a
// row computes what it computes in the one-clip call.  Nothing is recomputed and there is no halo.
//
// Kernels.  Rows are gathered from / scattered to the packed tensors by the table-driven copies of nc_ragged.hip, one launch per tensor
// and batch (a row's [n_q, T'] block is contiguous in both layouts).  A segmented Decode ends in ONE overlap_add_ragged_kernel launch
// that writes every clip from frames that live in different batch outputs; the decoded frames of all batches are kept in one arena
// until then; it stores through store_split16 (nc_copy.h).  All tables of a call are written (and bounds-checked) on the host before
// anything is launched and travel in one pinned image, copied once.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>

#include "nc_copy.h"
#include "nc_encodec_rows.h"
#include "nc_guard.h"
#include "nc_pool.h"
#include "nc_ragged.h"

namespace nc {

namespace {

// ---- overlap-add over all clips (OlaClip, OlaFrame, ola_sample, ola_eps: nc_encodec_rows.h) -----------------------------------------
// blockIdx.y = (clip, channel), blockIdx.x strides over its samples.  Memory-bound, no LDS, no atomics; the output row is stored by
// store_split16 (nc_copy.h) with ola_sample as its element; the frames are read at any alignment.
__global__ __launch_bounds__(256) void overlap_add_ragged_kernel(const OlaClip* __restrict__ clips, const OlaFrame* __restrict__ fr,
                                                                 const float* __restrict__ frames, int64_t stride, float* __restrict__ pcm) {
    const OlaClip d = clips[blockIdx.y];
    store_split16<float>(pcm + d.out, d.total, [&](int64_t t) { return ola_sample(d, fr, frames, stride, t); });
}

// ---- planner -----------------------------------------------------------------------------------------------------------------------
struct ErPlan {
    std::vector<ErRow> rows;          // launch order
    std::vector<ErBatch> batches;
    std::vector<int32_t> n_seg;       // per clip: segments, code frames, decoded samples
    std::vector<int64_t> frames, decoded;
    int64_t n_keys = 0, max_rows = 0, total_frames = 0, total_decoded = 0;
};

ErPlan make_plan(const EncodecModel& m, bool decode, int B, const int64_t* lengths, int32_t max_rows, const char* what) {
    if (!lengths) fail(NC_EINVAL, "%s: null pointer", what);
    if (B <= 0) fail(NC_EINVAL, "%s: B must be positive", what);
    ErPlan P;
    P.max_rows = er_max_rows(max_rows, what);
    for (int b = 0; b < B; ++b) {
        if (lengths[b] <= 0) fail(NC_EINVAL, "%s: clip %d has length %lld", what, b, (long long)lengths[b]);
        if (lengths[b] > ((int64_t)1 << 30)) fail(NC_EINVAL, "%s: clip %d: T must be at most 2^30", what, b);
        const std::vector<EncodecModel::Seg> segs = m.segments(lengths[b]);
        int64_t fr = 0;
        for (size_t s = 0; s < segs.size(); ++s) {
            const EncodecModel::Seg& g = segs[s];
            P.rows.push_back({b, (int32_t)s, g.off, decode ? m.decoded_for(g.frames) : g.len, g.frames, decode ? g.frames : g.len});
            fr += g.frames;
        }
        P.n_seg.push_back((int32_t)segs.size());
        P.frames.push_back(fr);
        P.decoded.push_back(m.decoded_len(segs));
        P.total_frames += fr;
        P.total_decoded += P.decoded.back();
    }
    P.n_keys = er_batches(P.rows, P.max_rows, P.batches);
    return P;
}

void report(const EncodecModel& m, const ErPlan& P, nc_encodec_ragged_plan* out, nc_encodec_ragged_row* rows, int64_t cap) {
    if (!out) fail(NC_EINVAL, "out must not be null");
    out->n_rows = (int64_t)P.rows.size(); out->n_keys = P.n_keys; out->n_batches = (int64_t)P.batches.size(); out->max_rows = P.max_rows;
    out->total_code_frames = P.total_frames; out->total_codes = (int64_t)m.n_q * P.total_frames; out->total_scales = (int64_t)P.rows.size();
    out->total_samples = P.total_decoded;
    if (!rows) return;
    for (size_t bi = 0; bi < P.batches.size(); ++bi)
        for (size_t r = P.batches[bi].first; r < P.batches[bi].first + P.batches[bi].count && (int64_t)r < cap; ++r) {
            const ErRow& w = P.rows[r];
            rows[r] = {w.clip, w.seg, (int32_t)bi, (int32_t)(r - P.batches[bi].first), w.off, w.len, w.frames};
        }
}

struct Offsets { std::vector<int64_t> samples, frames, rows, decoded; std::vector<int64_t> before; };   // prefix sums per clip; frames before a row within its clip
Offsets offsets_of(const ErPlan& P, int B, const int64_t* lengths) {
    Offsets o;
    o.samples.assign((size_t)B + 1, 0); o.frames = o.samples; o.rows = o.samples; o.decoded = o.samples;
    for (int b = 0; b < B; ++b) {
        o.samples[(size_t)b + 1] = o.samples[(size_t)b] + lengths[b];
        o.frames[(size_t)b + 1] = o.frames[(size_t)b] + P.frames[(size_t)b];
        o.rows[(size_t)b + 1] = o.rows[(size_t)b] + P.n_seg[(size_t)b];
        o.decoded[(size_t)b + 1] = o.decoded[(size_t)b] + P.decoded[(size_t)b];
    }
    // frames of the earlier segments of a row's clip: rows of a clip in segment order
    std::vector<int64_t> fr_of((size_t)o.rows.back(), 0);
    for (const ErRow& w : P.rows) fr_of[(size_t)(o.rows[(size_t)w.clip] + w.seg)] = w.frames;
    o.before.assign(fr_of.size(), 0);
    for (int b = 0; b < B; ++b)
        for (int64_t s = 1; s < P.n_seg[(size_t)b]; ++s)
            o.before[(size_t)(o.rows[(size_t)b] + s)] = o.before[(size_t)(o.rows[(size_t)b] + s - 1)] + fr_of[(size_t)(o.rows[(size_t)b] + s - 1)];
    return o;
}

}  // namespace

// ===================================================================================================================== Encode
void EncodecModel::encode_ragged_dev(const float* pcm, int B, const int64_t* lengths, int64_t* codes, float* scales, float* emb) {
    const char* what = "nc_encodec_encode_ragged";
    if (!pcm || !codes || !lengths) fail(NC_EINVAL, "%s: null pointer", what);
    const ErPlan P = make_plan(*this, false, B, lengths, ragged_rows, what);
    if (!loaded) fail(NC_ESTATE, "weights not loaded (call nc_codec_load_weights first)");
    er_check_rows(*this, P.rows, false, "clip", nullptr);
    const int C = cfg.channels, D = cfg.dimension, nq = n_q;
    const bool want_sc = cfg.normalize && scales;
    const Offsets o = offsets_of(P, B, lengths);
    const int64_t n_rows = (int64_t)P.rows.size();
    RgTables t;
    std::vector<size_t> first_launch;
    for (const ErBatch& bt : P.batches) {
        const int64_t N = (int64_t)bt.count, L = bt.key, Tz = P.rows[bt.first].frames;
        first_launch.push_back(t.launches.size());
        t.begin(C * o.samples.back(), N * C * L);   // one run per (row, channel): clip b is [C, T_b]
        for (int64_t r = 0; r < N; ++r) {
            const ErRow& w = P.rows[bt.first + (size_t)r];
            if (w.frames != Tz) fail(NC_ESTATE, "internal: rows of one key differ in frames");
            for (int c = 0; c < C; ++c) t.add(C * o.samples[(size_t)w.clip] + c * lengths[w.clip] + w.off, (r * C + c) * L, L);
        }
        t.end();
        t.begin(N * nq * Tz, nq * P.total_frames);
        for (int64_t r = 0; r < N; ++r) {
            const ErRow& w = P.rows[bt.first + (size_t)r];
            t.add(r * nq * Tz, nq * (o.frames[(size_t)w.clip] + o.before[(size_t)(o.rows[(size_t)w.clip] + w.seg)]), nq * Tz);
        }
        t.end();
        if (want_sc) {
            t.begin(N, n_rows);
            for (int64_t r = 0; r < N; ++r) t.add(r, o.rows[(size_t)P.rows[bt.first + (size_t)r].clip] + P.rows[bt.first + (size_t)r].seg, 1);
            t.end();
        }
        if (emb) {
            t.begin(N * D * Tz, D * P.total_frames);
            for (int64_t r = 0; r < N; ++r) {
                const ErRow& w = P.rows[bt.first + (size_t)r];
                t.add(r * D * Tz, D * (o.frames[(size_t)w.clip] + o.before[(size_t)(o.rows[(size_t)w.clip] + w.seg)]), D * Tz);
            }
            t.end();
        }
    }
    use_device();
    check_async_errors();   // an earlier device-pointer call on this handle may have timed out unnoticed
    LaneScope lanes(*this);
    rg_upload(*this, t);
    run_batches(er_assign_lanes(P.rows, P.batches), true, [&](size_t i) {
        const ErBatch& bt = P.batches[i];
        const int N = (int)bt.count;
        const int64_t L = bt.key, Tz = P.rows[bt.first].frames;
        size_t li = first_launch[i];
        float* x = alloc((size_t)N * C * L);
        int64_t* cb = reinterpret_cast<int64_t*>(alloc((size_t)N * nq * Tz * 2));
        float* sc = cfg.normalize ? alloc((size_t)N) : nullptr;
        float* eb = emb ? alloc((size_t)N * D * Tz) : nullptr;
        rg_copy_f32(*this, t, li++, pcm, x);
        encode_batch(x, N, L, Tz, cb, sc, eb);
        rg_copy_i64(*this, t, li++, cb, codes);
        if (want_sc) rg_copy_f32(*this, t, li++, sc, scales);
        if (emb) rg_copy_f32(*this, t, li++, eb, emb);
    });
}

// ===================================================================================================================== Decode
void EncodecModel::decode_ragged_dev(const int64_t* codes, const float* scales, int B, const int64_t* lengths, int nq, float* pcm) {
    const char* what = "nc_encodec_decode_ragged";
    if (!codes || !pcm || !lengths) fail(NC_EINVAL, "%s: null pointer", what);
    const ErPlan P = make_plan(*this, true, B, lengths, ragged_rows, what);
    if (!loaded) fail(NC_ESTATE, "weights not loaded (call nc_codec_load_weights first)");
    if (nq <= 0 || nq > cfg.n_codebooks) fail(NC_EINVAL, "codes carry %d codebooks; the model has %d", nq, cfg.n_codebooks);
    if (cfg.normalize && !scales) fail(NC_EINVAL, "this model normalises frames: scales must be given");
    er_check_rows(*this, P.rows, true, "clip", nullptr);
    const int C = cfg.channels;
    const bool segmented = cfg.segment_length > 0;
    const int64_t stride = cfg.segment_stride;
    const Offsets o = offsets_of(P, B, lengths);
    const int64_t n_rows = (int64_t)P.rows.size();
    RgTables t;
    std::vector<size_t> first_launch;
    std::vector<int64_t> arena_off;                               // of every batch's [N, C, Lo] output in the arena
    std::vector<OlaFrame> ftab((size_t)n_rows);                   // clip-major: frame f of clip b at rows[b] + f
    int64_t arena = 0;
    for (const ErBatch& bt : P.batches) {
        const int64_t N = (int64_t)bt.count, Tz = bt.key, Lo = P.rows[bt.first].len;
        first_launch.push_back(t.launches.size());
        t.begin(nq * P.total_frames, N * nq * Tz);
        for (int64_t r = 0; r < N; ++r) {
            const ErRow& w = P.rows[bt.first + (size_t)r];
            t.add(nq * (o.frames[(size_t)w.clip] + o.before[(size_t)(o.rows[(size_t)w.clip] + w.seg)]), r * nq * Tz, nq * Tz);
        }
        t.end();
        if (cfg.normalize) {
            t.begin(n_rows, N);
            for (int64_t r = 0; r < N; ++r) t.add(o.rows[(size_t)P.rows[bt.first + (size_t)r].clip] + P.rows[bt.first + (size_t)r].seg, r, 1);
            t.end();
        }
        if (!segmented) {   // single frame: DecodeFrame output as is
            t.begin(N * C * Lo, C * P.total_decoded);
            for (int64_t r = 0; r < N; ++r) t.add(r * C * Lo, C * o.decoded[(size_t)P.rows[bt.first + (size_t)r].clip], C * Lo);
            t.end();
        } else {
            arena_off.push_back(arena);
            for (int64_t r = 0; r < N; ++r) {
                const ErRow& w = P.rows[bt.first + (size_t)r];
                ftab[(size_t)(o.rows[(size_t)w.clip] + w.seg)] = {arena + r * C * Lo, Lo, Lo};
            }
            arena += N * C * Lo;
        }
    }
    std::vector<OlaClip> ctab;
    int64_t longest = 1;
    if (segmented) {
        for (int b = 0; b < B; ++b) {
            const int64_t first = o.rows[(size_t)b];
            const int nfr = P.n_seg[(size_t)b];
            std::vector<int64_t> flen((size_t)nfr);
            for (int f = 0; f < nfr; ++f) {
                const OlaFrame& g = ftab[(size_t)(first + f)];
                if (g.off < 0 || g.len <= 0 || g.off + C * g.len > arena) fail(NC_ESTATE, "internal: frame %d of clip %d leaves the arena", f, b);
                flen[(size_t)f] = g.len;
                if (g.len > flen[0]) fail(NC_EINVAL, "clip %d: a later frame is longer than the first one", b);
            }
            const int64_t total = stride * (nfr - 1) + flen[(size_t)nfr - 1];
            if (total != P.decoded[(size_t)b]) fail(NC_ESTATE, "internal: clip %d overlap-adds to %lld samples, planned %lld", b, (long long)total, (long long)P.decoded[(size_t)b]);
            const float eps = ola_eps(flen, stride, total);
            for (int c = 0; c < C; ++c) ctab.push_back({C * o.decoded[(size_t)b] + c * total, total, first, flen[0], nfr, c, eps, 0});
            longest = std::max(longest, total);
        }
        t.extra.resize(ctab.size() * sizeof(OlaClip) + ftab.size() * sizeof(OlaFrame));
        std::memcpy(t.extra.data(), ctab.data(), ctab.size() * sizeof(OlaClip));
        std::memcpy(t.extra.data() + ctab.size() * sizeof(OlaClip), ftab.data(), ftab.size() * sizeof(OlaFrame));
    }
    use_device();
    check_async_errors();
    LaneScope lanes(*this);
    if (segmented) rg_frames.reserve((size_t)arena * 4);
    const char* extra = rg_upload(*this, t);
    run_batches(er_assign_lanes(P.rows, P.batches), true, [&](size_t i) {
        const ErBatch& bt = P.batches[i];
        const int N = (int)bt.count;
        const int64_t Tz = bt.key, Lo = P.rows[bt.first].len;
        size_t li = first_launch[i];
        int64_t* cb = reinterpret_cast<int64_t*>(alloc((size_t)N * nq * Tz * 2));
        float* sc = cfg.normalize ? alloc((size_t)N) : nullptr;
        rg_copy_i64(*this, t, li++, codes, cb);
        if (sc) rg_copy_f32(*this, t, li++, scales, sc);
        int64_t got = 0;
        const float* out = decode_batch(cb, N, nq, Tz, sc, &got);
        if (got != Lo) fail(NC_ESTATE, "internal: decoder produced %lld samples, planned %lld", (long long)got, (long long)Lo);
        if (!segmented) rg_copy_f32(*this, t, li++, out, pcm);
        else NC_HIP(hipMemcpyAsync(rg_frames.as<float>() + arena_off[i], out, (size_t)N * C * Lo * 4, hipMemcpyDeviceToDevice, stream));
    });
    if (!segmented) return;
    const OlaClip* dct = reinterpret_cast<const OlaClip*>(extra);
    const OlaFrame* dft = reinterpret_cast<const OlaFrame*>(extra + ctab.size() * sizeof(OlaClip));
    const unsigned gx = copy_grid_x(longest, 4);
    for_grid_y(ctab.size(), [&](size_t done, size_t cnt) {
        ProfScope ps(&prof, stream, NC_KC_ELEM, 0.0, 8.0 * (double)C * (double)P.total_decoded);
        hipLaunchKernelGGL(overlap_add_ragged_kernel, dim3(gx, (unsigned)cnt), dim3(256), 0, stream, dct + done, dft, rg_frames.as<float>(), stride, pcm);
        NC_HIP(hipGetLastError());
    });
}

}  // namespace nc

// ================================================================================================ C ABI
using namespace nc;

extern "C" {

nc_status nc_encodec_ragged_rows(const nc_encodec_config* cfg, int32_t decode, int32_t B, const int64_t* lengths, int32_t max_rows,
                                 nc_encodec_ragged_plan* out, nc_encodec_ragged_row* rows, int64_t cap) {
    return guard([&] {
        if (!cfg) fail(NC_EINVAL, "cfg must not be null");
        const EncodecModel m(*cfg);   // host arithmetic alone: no device is touched
        report(m, make_plan(m, decode != 0, B, lengths, max_rows, "nc_encodec_ragged_rows"), out, rows, cap);
    });
}

nc_status nc_encodec_set_ragged_rows(nc_codec* h, int32_t max_rows) {
    return guard([&] {
        EncodecModel& m = as<EncodecModel>(h);
        if (max_rows < 0 || max_rows > EncodecModel::RAGGED_MAX_ROWS) fail(NC_EINVAL, "max_rows must be 0 (default) .. %d", EncodecModel::RAGGED_MAX_ROWS);
        m.ragged_rows = max_rows;
    });
}

nc_status nc_encodec_ragged_rows_of(const nc_codec* h, int32_t decode, int32_t B, const int64_t* lengths, nc_encodec_ragged_plan* out,
                                    nc_encodec_ragged_row* rows, int64_t cap) {
    return guard([&] {
        EncodecModel& m = as<EncodecModel>(h);
        report(m, make_plan(m, decode != 0, B, lengths, m.ragged_rows, "nc_encodec_ragged_rows_of"), out, rows, cap);
    });
}

nc_status nc_encodec_ragged_query(const nc_codec* h, int32_t B, const int64_t* lengths, int32_t* n_frames, int64_t* code_frames, int64_t* decoded_lens) {
    return guard([&] {
        EncodecModel& m = as<EncodecModel>(h);
        const ErPlan P = make_plan(m, false, B, lengths, m.ragged_rows, "nc_encodec_ragged_query");
        for (int b = 0; b < B; ++b) {
            if (n_frames) n_frames[b] = P.n_seg[(size_t)b];
            if (code_frames) code_frames[b] = P.frames[(size_t)b];
            if (decoded_lens) decoded_lens[b] = P.decoded[(size_t)b];
        }
    });
}

nc_status nc_encodec_encode_ragged_dev(nc_codec* h, const float* pcm_packed, int32_t B, const int64_t* lengths, int64_t* codes_packed,
                                       float* scales_packed, float* emb_packed) {
    return guard([&] { as<EncodecModel>(h).encode_ragged_dev(pcm_packed, B, lengths, codes_packed, scales_packed, emb_packed); });
}

nc_status nc_encodec_decode_ragged_dev(nc_codec* h, const int64_t* codes_packed, const float* scales_packed, int32_t B, const int64_t* lengths,
                                       int32_t n_q, float* pcm_packed) {
    return guard([&] { as<EncodecModel>(h).decode_ragged_dev(codes_packed, scales_packed, B, lengths, n_q, pcm_packed); });
}

nc_status nc_encodec_encode_ragged(nc_codec* h, const float* pcm_packed, int32_t B, const int64_t* lengths, int64_t* codes_packed,
                                   float* scales_packed, float* emb_packed) {
    return guard([&] {
        EncodecModel& m = as<EncodecModel>(h);
        const char* what = "nc_encodec_encode_ragged";
        if (!pcm_packed || !codes_packed || !lengths) fail(NC_EINVAL, "%s: null pointer", what);
        const ErPlan P = make_plan(m, false, B, lengths, m.ragged_rows, what);
        if (!m.loaded) fail(NC_ESTATE, "weights not loaded (call nc_codec_load_weights first)");
        er_check_rows(m, P.rows, false, "clip", nullptr);   // every refusal before the first copy
        int64_t samples = 0;
        for (int b = 0; b < B; ++b) samples += lengths[b];
        const size_t n_in = (size_t)m.cfg.channels * samples * 4, n_codes = (size_t)m.n_q * P.total_frames * 8, n_sc = P.rows.size() * 4,
                     n_emb = (size_t)m.cfg.dimension * P.total_frames * 4;
        m.use_device();
        OwnStreamScope own(m);
        m.rg_out.reserve(n_codes); m.ck_b.reserve(n_sc);
        if (emb_packed) m.ck_out.reserve(n_emb);
        h2d(m.rg_in, pcm_packed, n_in, m.stream);
        encodec_host_run(m, [&] {
            m.encode_ragged_dev(m.rg_in.as<float>(), B, lengths, m.rg_out.as<int64_t>(), m.ck_b.as<float>(), emb_packed ? m.ck_out.as<float>() : nullptr);
        });
        NC_HIP(hipMemcpyAsync(codes_packed, m.rg_out.p, n_codes, hipMemcpyDeviceToHost, m.stream));
        if (scales_packed && m.cfg.normalize) NC_HIP(hipMemcpyAsync(scales_packed, m.ck_b.p, n_sc, hipMemcpyDeviceToHost, m.stream));
        if (emb_packed) NC_HIP(hipMemcpyAsync(emb_packed, m.ck_out.p, n_emb, hipMemcpyDeviceToHost, m.stream));
        NC_HIP(hipStreamSynchronize(m.stream));
    });
}

nc_status nc_encodec_decode_ragged(nc_codec* h, const int64_t* codes_packed, const float* scales_packed, int32_t B, const int64_t* lengths,
                                   int32_t n_q, float* pcm_packed) {
    return guard([&] {
        EncodecModel& m = as<EncodecModel>(h);
        const char* what = "nc_encodec_decode_ragged";
        if (!codes_packed || !pcm_packed || !lengths) fail(NC_EINVAL, "%s: null pointer", what);
        const ErPlan P = make_plan(m, true, B, lengths, m.ragged_rows, what);
        if (!m.loaded) fail(NC_ESTATE, "weights not loaded (call nc_codec_load_weights first)");
        if (n_q <= 0 || n_q > m.cfg.n_codebooks) fail(NC_EINVAL, "codes carry %d codebooks; the model has %d", n_q, m.cfg.n_codebooks);
        if (m.cfg.normalize && !scales_packed) fail(NC_EINVAL, "this model normalises frames: scales must be given");
        er_check_rows(m, P.rows, true, "clip", nullptr);
        const size_t n_codes = (size_t)n_q * P.total_frames * 8, n_sc = P.rows.size() * 4, n_out = (size_t)m.cfg.channels * P.total_decoded * 4;
        m.use_device();
        OwnStreamScope own(m);
        m.rg_out.reserve(n_out);
        h2d(m.rg_in, codes_packed, n_codes, m.stream);
        if (scales_packed) h2d(m.ck_a, scales_packed, n_sc, m.stream);
        encodec_host_run(m, [&] {
            m.decode_ragged_dev(m.rg_in.as<int64_t>(), scales_packed ? m.ck_a.as<float>() : nullptr, B, lengths, n_q, m.rg_out.as<float>());
        });
        NC_HIP(hipMemcpyAsync(pcm_packed, m.rg_out.p, n_out, hipMemcpyDeviceToHost, m.stream));
        NC_HIP(hipStreamSynchronize(m.stream));
    });
}

}  // extern "C"
