// Encodec stream pool: Encode / Decode of many live streams, segment by segment as PCM or frames arrive (include/nc_mi355x.h, "Encodec
// stream pool").  Segmented models only: a segment depends on nothing outside itself (nc_encodec_ragged.hip), so the state between two
// calls is small and is not model state at all --
//   Encode   the samples from the next segment's start on (fewer than segment_length per channel);
//   Decode   the raw tail of the last full frame, its last decoded(F_full) - stride samples, which the next frame overlaps.
// Planner.  A row is one (entry, segment) pair of this step, its key the segment's sample count (Encode) or code-frame count (Decode);
// rows of equal key from any slots form batches of at most max_rows rows and run through the unchanged encode_batch / decode_batch, keys
// in descending order -- the ragged calls' grouping, so a lock-step step of n streams is one n-row launch sequence.
// Why it is exact: a row computes what it computes in the one-clip call (the batch invariance the ragged calls rest on); the rows of a
// stream are the segments of the whole clip, each emitted once, in order (tests/test_encodec_stream_plan_cpu.py); and an output sample
// of the overlap-add is ola_sample (nc_encodec_rows.h) over the same frames in the same order as in the ragged kernel, which equals the
// one-clip call -- a sample is final once the frames that can cover it have arrived, and with decoded(F_full) <= 2 * stride those are
// the frame it starts in and the one before, whose tail is the carry.
// Kernels.  encodec_stream_gather_kernel: one launch per Encode step assembles every row of every batch from the slot's carry and the
// entry's new PCM and writes every pushing slot's new carry.  overlap_add_stream_kernel: one launch per Decode step over all (entry,
// channel) pairs writes the final samples and the new carry.  Both read one half of a slot's carry and write the other (the step then
// flips the slot), so no thread reads what another thread of the launch writes; vector stores only, no atomics.  Both store through the
// shared copy body (nc_copy.h); the pool's host scaffold -- two-half carry, slot lookup, a step's state refusals, host-pointer staging --
// is nc_pool.h.  All tables of a step are written and bounds-checked on the host before anything is launched and travel in one pinned
// image (nc_ragged.h).
#include <algorithm>
#include <cstring>

#include "nc_copy.h"
#include "nc_encodec_rows.h"
#include "nc_guard.h"
#include "nc_pool.h"
#include "nc_ragged.h"

using namespace nc;

namespace {

// ---- tables ------------------------------------------------------------------------------------------------------------------------
// One run of the gather: dst[i] = i < a_n ? carry[a_src + i] : pcm[b_src + i - a_n] for i < a_n + b_n; dst is the batch arena
// (to_carry == 0) or the carry buffer.  Elements.
struct EsRun { int64_t dst, a_src, a_n, b_src, b_n, to_carry; };
// One (entry, channel) of the overlap-add: output samples t0 .. clip.total - 1 of the entry's frame list (the carried frame, if any,
// then this step's frames) go to pcm[clip.out + (t - t0)]; then carry_n elements of the frames' buffer are copied from carry_src to
// carry_dst (the last full frame's tail to the slot's other half).
struct EsOla { OlaClip clip; int64_t t0, carry_dst, carry_src, carry_n; };

// ---- kernels -----------------------------------------------------------------------------------------------------------------------
// blockIdx.y = run, blockIdx.x strides over it.  Memory-bound, no LDS, no atomics; a run is one concat_copy (nc_copy.h).  carry_in and
// carry_out are the same buffer, so neither is __restrict__ here: a run reads one half of a slot and writes the other, or appends behind
// what the slot holds.
__global__ __launch_bounds__(256) void encodec_stream_gather_kernel(const EsRun* __restrict__ runs, const float* carry_in, const float* __restrict__ pcm,
                                                                    float* __restrict__ x, float* carry_out) {
    const EsRun g = runs[blockIdx.y];
    concat_copy<float>(carry_in + g.a_src, g.a_n, pcm + g.b_src, g.b_n, 0, (g.to_carry ? carry_out : x) + g.dst, g.a_n + g.b_n);
}

// blockIdx.y = (entry, channel), blockIdx.x strides over its samples and then over its carry.  The samples are stored as in
// overlap_add_ragged_kernel, ola_sample being the element; the carry is a concat_copy of one piece.  `frames` holds the carry halves of
// every slot in front of this step's decoded frames: the samples read the slot's current half and the arena, the copy writes the other half.
__global__ __launch_bounds__(256) void overlap_add_stream_kernel(const EsOla* __restrict__ jobs, const OlaFrame* __restrict__ fr, float* frames, int64_t stride,
                                                                 float* __restrict__ pcm) {
    const EsOla j = jobs[blockIdx.y];
    const OlaClip d = j.clip;
    store_split16<float>(pcm + d.out, d.total - j.t0, [&](int64_t t) { return ola_sample(d, fr, frames, stride, j.t0 + t); });
    concat_copy<float>(frames + j.carry_src, j.carry_n, nullptr, 0, 0, frames + j.carry_dst, j.carry_n);
}

// ---- planner -----------------------------------------------------------------------------------------------------------------------
struct EsGeom {
    int64_t seg = 0, stride = 0, F_full = 0, L_full = 0, ov = 0;   // ov = L_full - stride: the decoded tail the next frame overlaps
};

// NC_EUNSUPPORTED where a stream cannot be cut: no segmentation; and, for the layouts no preset has, where the state above is not all
EsGeom geom_of(const EncodecModel& m, const char* what) {
    EsGeom g;
    if (m.cfg.segment_length <= 0)
        fail(NC_EUNSUPPORTED, "%s: this model is not segmented (segment_length == 0: the 24 kHz preset) -- its LSTM runs over the whole clip, so no "
                              "part of a stream stands for the stream; the stream pool serves segmented models (48 kHz) only", what);
    g.seg = m.cfg.segment_length; g.stride = m.cfg.segment_stride;
    if (g.stride <= 0 || g.stride >= g.seg) fail(NC_EUNSUPPORTED, "%s: segment_stride must be in 1 .. segment_length - 1", what);
    g.F_full = m.frames_for(g.seg);
    g.L_full = m.decoded_for(g.F_full);
    g.ov = g.L_full - g.stride;
    if (g.L_full > 2 * g.stride) fail(NC_EUNSUPPORTED, "%s: a full frame decodes to more than two strides: more than two frames overlap", what);
    // the window's ends round to zero beyond 2^25 samples and the overlap-add's `+ 1e-10` branch could be taken (ola_eps): not carried
    if (g.L_full > ((int64_t)1 << 25)) fail(NC_EUNSUPPORTED, "%s: segments of more than 2^25 decoded samples are not streamed", what);
    return g;
}

// the last one or two frames of a layout, as nc_encodec_clip_length decides it: some tail of 1 .. stride samples gives these frame counts
bool tail_layout_ok(const EncodecModel& m, const EsGeom& g, int n, const int64_t* lens) {
    for (int64_t tail = 1; tail <= g.stride; ++tail) {
        if (m.frames_for(std::min(tail, g.seg)) != lens[n - 1]) continue;
        if (n == 1 || m.frames_for(std::min(g.seg, g.stride + tail)) == lens[0]) return true;
    }
    return false;
}

struct EsEntry {
    int32_t id = 0;                      // the slot (pool) or the stream's index (planner)
    int64_t T0 = 0, next0 = 0;           // before the step: samples | frames received; Encode: segments emitted
    int64_t n_in = 0;
    bool flush = false;
    int64_t T1 = 0, next1 = 0;           // after it
    int32_t n_rows = 0;
    int64_t code_frames = 0, n_samples = 0;
    int64_t in_off = 0, row_off = 0, out_off = 0;   // prefix sums over the entries: samples | code frames in, rows, code frames | samples out
    std::vector<int64_t> flen;           // code frames of the entry's rows in segment order
    std::vector<int64_t> before;         // ... summed over the earlier ones
    std::vector<std::pair<int, int>> at; // (batch, row) of every row, filled once the batches stand
};
struct EsPlan {
    std::vector<EsEntry> e;
    std::vector<ErRow> rows;
    std::vector<ErBatch> batches;
    int64_t n_keys = 0, max_rows = 0, total_in = 0, total_frames = 0, total_samples = 0;
};

EsPlan make_plan(const EncodecModel& m, const EsGeom& g, bool decode, int n, const int32_t* ids, const int64_t* T0, const int64_t* next0, const int64_t* n_in,
                 const int32_t* flush, const int64_t* frame_lens, int32_t max_rows, const char* what) {
    EsPlan P;
    P.max_rows = er_max_rows(max_rows, what);
    P.e.resize((size_t)n);
    int64_t lens_at = 0, n_rows = 0;
    for (int i = 0; i < n; ++i) {
        EsEntry& e = P.e[(size_t)i];
        e.id = ids ? ids[i] : i;
        e.T0 = T0[i]; e.next0 = next0[i]; e.n_in = n_in[i]; e.flush = flush && flush[i] != 0;
        if (e.n_in < 0) fail(NC_EINVAL, "%s: slot %d: n_in is negative", what, e.id);
        if (e.n_in > ((int64_t)1 << 30) || e.T0 > ((int64_t)1 << 40)) fail(NC_EINVAL, "%s: slot %d: stream too long", what, e.id);
        e.T1 = e.T0 + e.n_in;
        if (e.flush && e.T1 == 0) fail(NC_EINVAL, "%s: slot %d: a flush of a stream that has received nothing", what, e.id);
        e.in_off = P.total_in; e.row_off = n_rows;
        if (!decode) {
            int64_t k = e.next0;
            for (; k * g.stride + g.seg <= e.T1; ++k) { P.rows.push_back({i, (int32_t)k, k * g.stride, g.seg, g.F_full, g.seg}); e.flen.push_back(g.F_full); }
            e.next1 = k;
            e.n_samples = e.T1 - k * g.stride;   // kept; at least the overlap once a segment has been emitted, never a whole segment
            if (e.flush) {                       // the rest of segments(T1): Encodec.cs:278-282
                for (; k * g.stride < e.T1; ++k) {
                    const int64_t len = std::min(g.seg, e.T1 - k * g.stride), fr = m.frames_for(len);
                    P.rows.push_back({i, (int32_t)k, k * g.stride, len, fr, len});
                    e.flen.push_back(fr);
                }
                e.n_samples = 0;
            }
            P.total_in += m.cfg.channels * e.n_in;
        } else {
            std::vector<int64_t> lens((size_t)e.n_in, g.F_full);
            if (frame_lens) std::copy(frame_lens + lens_at, frame_lens + lens_at + e.n_in, lens.begin());
            lens_at += e.n_in;
            const int64_t n_full = e.flush ? std::max<int64_t>(0, e.T1 - 2) - e.T0 : e.n_in;   // frames of this entry that must be full
            for (int64_t j = 0; j < e.n_in; ++j) {
                if (lens[(size_t)j] <= 0) fail(NC_EINVAL, "%s: slot %d: a frame without codes", what, e.id);
                if (j < n_full && lens[(size_t)j] != g.F_full)
                    fail(NC_EINVAL, "%s: slot %d: frame %lld holds %lld code frames, a full segment has %lld (only the last two frames of a flush may be short)", what,
                         e.id, (long long)(e.T0 + j), (long long)lens[(size_t)j], (long long)g.F_full);
            }
            int64_t last = g.F_full, first = e.T0 > 0 || e.n_in == 0 ? g.F_full : lens[0];
            if (e.flush) {   // the last two frames of the whole list: earlier pushes brought full frames
                int64_t two[2];
                const int cnt = (int)std::min<int64_t>(2, e.T1);
                for (int q = 0; q < cnt; ++q) {
                    const int64_t f = e.T1 - cnt + q;   // frame index in the stream
                    two[q] = f < e.T0 ? g.F_full : lens[(size_t)(f - e.T0)];
                }
                if (!tail_layout_ok(m, g, cnt, two))
                    fail(NC_EINVAL, "%s: slot %d: no clip length yields this layout of %lld segments (%lld code frames in the last)", what, e.id, (long long)e.T1,
                         (long long)two[cnt - 1]);
                last = two[cnt - 1];
            }
            for (int64_t j = 0; j < e.n_in; ++j) {
                if (lens[(size_t)j] > first) fail(NC_EINVAL, "%s: slot %d: a later frame is longer than the first one", what, e.id);
                P.rows.push_back({i, (int32_t)(e.T0 + j), (e.T0 + j) * g.stride, m.decoded_for(lens[(size_t)j]), lens[(size_t)j], lens[(size_t)j]});
                e.flen.push_back(lens[(size_t)j]);
            }
            e.n_samples = e.flush ? (e.T1 - 1) * g.stride + m.decoded_for(last) - e.T0 * g.stride : e.n_in * g.stride;
            P.total_samples += e.n_samples;
        }
        e.n_rows = (int32_t)e.flen.size();
        e.before.assign(e.flen.size(), 0);
        for (size_t r = 0; r < e.flen.size(); ++r) {
            e.before[r] = e.code_frames;
            e.code_frames += e.flen[r];
        }
        if (decode) { P.total_in += e.code_frames; e.out_off = P.total_samples - e.n_samples; }
        else e.out_off = P.total_frames;
        P.total_frames += e.code_frames;
        n_rows += e.n_rows;
    }
    P.n_keys = P.rows.empty() ? 0 : er_batches(P.rows, P.max_rows, P.batches);
    for (EsEntry& e : P.e) e.at.assign(e.flen.size(), {-1, -1});
    for (size_t bi = 0; bi < P.batches.size(); ++bi)
        for (size_t r = 0; r < P.batches[bi].count; ++r) {
            const ErRow& w = P.rows[P.batches[bi].first + r];
            EsEntry& e = P.e[(size_t)w.clip];
            e.at[(size_t)(w.seg - (decode ? e.T0 : e.next0))] = {(int)bi, (int)r};
        }
    return P;
}

void report(const EncodecModel& m, int nq, const EsPlan& P, nc_encodec_ragged_plan* out, nc_encodec_ragged_row* rows, int64_t cap, int32_t* n_frames,
            int64_t* code_frames, int64_t* n_samples) {
    if (out) {
        out->n_rows = (int64_t)P.rows.size(); out->n_keys = P.n_keys; out->n_batches = (int64_t)P.batches.size(); out->max_rows = P.max_rows;
        out->total_code_frames = P.total_frames; out->total_codes = (int64_t)nq * P.total_frames; out->total_scales = (int64_t)P.rows.size();
        out->total_samples = P.total_samples;
    }
    if (rows)
        for (size_t bi = 0; bi < P.batches.size(); ++bi)
            for (size_t r = P.batches[bi].first; r < P.batches[bi].first + P.batches[bi].count && (int64_t)r < cap; ++r) {
                const ErRow& w = P.rows[r];
                rows[r] = {w.clip, w.seg, (int32_t)bi, (int32_t)(r - P.batches[bi].first), w.off, w.len, w.frames};
            }
    for (size_t i = 0; i < P.e.size(); ++i) {
        if (n_frames) n_frames[i] = P.e[i].n_rows;
        if (code_frames) code_frames[i] = P.e[i].code_frames;
        if (n_samples) n_samples[i] = P.e[i].n_samples;
    }
}

}  // namespace

// ===================================================================================================================== the pool
struct nc_encodec_stream_pool {
    nc_codec* h = nullptr;
    bool decode = false;
    int nq = 0;                          // Decode: codebooks in the pushed codes
    EsGeom g;
    struct Slot {
        int64_t T = 0;                   // samples (Encode) or frames (Decode) received
        int64_t next = 0;                // Encode: the next segment to emit
        bool ended = false;
        int cur = 0;                     // the half of the carry that holds the slot's state
    };
    std::vector<Slot> slots;
    TwoHalves halves;                    // of the carry; per slot and half: Encode [channels][segment_length], Decode [channels][ov]
    // Encode: `carry` is [2][n_slots][cap], `arena` the dense inputs of every batch of a step.  Decode: `arena` is the carry halves
    // followed by the decoded frames of every batch of a step -- one buffer, the frames' base of ola_sample.
    DevBuf carry, arena;
    DevBuf in_stage, sc_stage, out_stage, sc_out, emb_stage;   // the packed tensors of a host-pointer call

    EncodecModel& model() const { return as<EncodecModel>(h); }
    int64_t n_slots() const { return (int64_t)slots.size(); }
    static constexpr const char* kNull = "null stream pool";
    static constexpr const char* kRange = kSlotOutOfRange;
    static constexpr int kRangeLast = 0;

    EsPlan plan(int n, const int32_t* ids, const int64_t* n_in, const int32_t* flush, const int64_t* frame_lens, const char* what) const;
    void check(const EsPlan& P) const;
    void grow_arena(EncodecModel& m, int64_t elems);
    void step_dev(const EsPlan& P, const void* in, const float* scales_in, void* out, float* scales_out, float* emb);
    void encode_dev(EncodecModel& m, const EsPlan& P, const float* pcm, int64_t* codes, float* scales, float* emb);
    void decode_dev(EncodecModel& m, const EsPlan& P, const int64_t* codes, const float* scales, float* pcm);
    void commit(const EsPlan& P);
};

// every refusal that needs the slots' state, then the plan (which refuses the rest); nothing is changed
EsPlan nc_encodec_stream_pool::plan(int n, const int32_t* ids, const int64_t* n_in, const int32_t* flush, const int64_t* frame_lens, const char* what) const {
    std::vector<int64_t> T0, next0;
    pool_named_slots(*this, n, ids, n_in, what, &Slot::next, T0, next0);
    const EncodecModel& m = model();
    return make_plan(m, g, decode, n, ids, T0.data(), next0.data(), n_in, flush, frame_lens, m.ragged_rows, what);
}

// what the launch sequences would refuse on a row, with the slot's name
void nc_encodec_stream_pool::check(const EsPlan& P) const {
    const EncodecModel& m = model();
    if (!m.loaded) fail(NC_ESTATE, "weights not loaded (call nc_codec_load_weights first)");
    std::vector<int32_t> ids;
    for (const EsEntry& e : P.e) ids.push_back(e.id);
    er_check_rows(m, P.rows, decode, "slot", ids.data());
}

// Decode: the carry halves live in front of the frames and survive a larger arena
void nc_encodec_stream_pool::grow_arena(EncodecModel& m, int64_t elems) {
    if ((size_t)elems * 4 <= arena.cap) return;
    if (!decode || !arena.p) { arena.reserve((size_t)elems * 4); return; }
    DevBuf big;
    big.reserve((size_t)elems * 4);
    NC_HIP(hipMemcpyAsync(big.p, arena.p, (size_t)halves.elems() * 4, hipMemcpyDeviceToDevice, m.stream));
    NC_HIP(hipStreamSynchronize(m.stream));   // (earlier steps on this stream still read the old buffer)
    arena = std::move(big);
}

void nc_encodec_stream_pool::commit(const EsPlan& P) {
    for (const EsEntry& e : P.e) {
        Slot& s = slots[(size_t)e.id];
        const bool rewrote = decode ? e.n_in > 0 : e.next1 != e.next0;   // the step wrote the slot's other half
        s.T = e.T1; s.next = e.next1;
        if (e.flush) s.ended = true;
        else if (rewrote) s.cur ^= 1;
    }
}

void nc_encodec_stream_pool::step_dev(const EsPlan& P, const void* in, const float* scales_in, void* out, float* scales_out, float* emb) {
    EncodecModel& m = model();
    m.use_device();
    m.check_async_errors();   // an earlier device-pointer call on this handle may have timed out unnoticed
    if (decode) decode_dev(m, P, static_cast<const int64_t*>(in), scales_in, static_cast<float*>(out));
    else encode_dev(m, P, static_cast<const float*>(in), static_cast<int64_t*>(out), scales_out, emb);
}

// ===================================================================================================================== Encode
void nc_encodec_stream_pool::encode_dev(EncodecModel& m, const EsPlan& P, const float* pcm, int64_t* codes, float* scales, float* emb) {
    const int C = m.cfg.channels, D = m.cfg.dimension, nqe = m.n_q;
    const bool want_sc = m.cfg.normalize && scales;
    const int64_t n_rows = (int64_t)P.rows.size();
    // the batches' dense inputs in the arena
    std::vector<int64_t> x_off;
    int64_t x_total = 0;
    for (const ErBatch& bt : P.batches) { x_off.push_back(x_total); x_total += round_up((int64_t)bt.count * C * bt.key, kAlign); }
    // gather runs: the rows of every batch, then the new carries
    std::vector<EsRun> runs;
    int64_t longest = 1;
    auto add_run = [&](const EsEntry& e, int c, int64_t g0, int64_t len, int64_t dst, bool to_carry, int64_t dst_elems) {
        // [g0, g0 + len) of the stream: [next0 * stride, T0) is in the slot's current half, [T0, T1) in the entry's PCM
        const int64_t c0 = e.next0 * g.stride, held = e.T0 - c0;
        const int64_t a_n = std::min(len, std::max<int64_t>(0, e.T0 - g0)), b_n = len - a_n;
        const int64_t a_src = halves.at(slots[(size_t)e.id].cur, e.id) + (int64_t)c * g.seg + (g0 - c0);
        const int64_t b_src = e.in_off + (int64_t)c * e.n_in + (g0 + a_n - e.T0);
        if (len <= 0 || g0 < c0 || g0 + len > e.T1 || held < 0 || held > g.seg || (a_n && g0 - c0 + a_n > held) || (b_n && (b_src < e.in_off || b_src + b_n > e.in_off + (int64_t)C * e.n_in)) ||
            dst < 0 || dst + len > dst_elems)
            fail(NC_ESTATE, "internal: slot %d: a gather run leaves its tensors", e.id);
        runs.push_back({dst, a_n ? a_src : 0, a_n, b_n ? b_src : 0, b_n, to_carry ? 1 : 0});
        longest = std::max(longest, len);
    };
    for (size_t bi = 0; bi < P.batches.size(); ++bi) {
        const ErBatch& bt = P.batches[bi];
        for (size_t r = 0; r < bt.count; ++r) {
            const ErRow& w = P.rows[bt.first + r];
            for (int c = 0; c < C; ++c) add_run(P.e[(size_t)w.clip], c, w.off, w.len, x_off[bi] + ((int64_t)r * C + c) * bt.key, false, x_total);
        }
    }
    for (const EsEntry& e : P.e) {
        if (e.flush || e.n_in == 0) continue;
        const Slot& s = slots[(size_t)e.id];
        for (int c = 0; c < C; ++c) {
            if (e.next1 != e.next0) {   // segments went out: what is kept, into the other half
                const int64_t base = halves.at(s.cur ^ 1, e.id);
                add_run(e, c, e.next1 * g.stride, e.n_samples, base + (int64_t)c * g.seg, true, base + halves.cap);
            } else {                    // nothing went out: the push is appended behind what the slot holds
                const int64_t base = halves.at(s.cur, e.id);
                add_run(e, c, e.T0, e.n_in, base + (int64_t)c * g.seg + (e.T0 - e.next0 * g.stride), true, base + (int64_t)(c + 1) * g.seg);
            }
        }
    }
    // the batches' outputs to the packed tensors
    RgTables t;
    std::vector<size_t> first_launch;
    for (const ErBatch& bt : P.batches) {
        const int64_t N = (int64_t)bt.count, Tz = P.rows[bt.first].frames;
        first_launch.push_back(t.launches.size());
        auto dst_frames = [&](const ErRow& w) { const EsEntry& e = P.e[(size_t)w.clip]; return e.out_off + e.before[(size_t)(w.seg - e.next0)]; };
        t.begin(N * nqe * Tz, nqe * P.total_frames);
        for (int64_t r = 0; r < N; ++r) {
            const ErRow& w = P.rows[bt.first + (size_t)r];
            if (w.frames != Tz) fail(NC_ESTATE, "internal: rows of one key differ in frames");
            t.add(r * nqe * Tz, nqe * dst_frames(w), nqe * Tz);
        }
        t.end();
        if (want_sc) {
            t.begin(N, n_rows);
            for (int64_t r = 0; r < N; ++r) {
                const ErRow& w = P.rows[bt.first + (size_t)r];
                t.add(r, P.e[(size_t)w.clip].row_off + (w.seg - P.e[(size_t)w.clip].next0), 1);
            }
            t.end();
        }
        if (emb) {
            t.begin(N * D * Tz, D * P.total_frames);
            for (int64_t r = 0; r < N; ++r) t.add(r * D * Tz, D * dst_frames(P.rows[bt.first + (size_t)r]), D * Tz);
            t.end();
        }
    }
    if (runs.empty()) return;   // (an entry that pushes nothing and flushes nothing)
    t.extra.resize(runs.size() * sizeof(EsRun));
    std::memcpy(t.extra.data(), runs.data(), t.extra.size());
    arena.reserve((size_t)std::max<int64_t>(x_total, 4) * 4);
    LaneScope lanes(m);
    const EsRun* druns = reinterpret_cast<const EsRun*>(rg_upload(m, t));
    const unsigned gx = copy_grid_x(longest, 4);
    for_grid_y(runs.size(), [&](size_t done, size_t cnt) {
        double bytes = 0;
        if (m.prof.on)
            for (size_t i = 0; i < cnt; ++i) bytes += 8.0 * (double)(runs[done + i].a_n + runs[done + i].b_n);
        ProfScope ps(&m.prof, m.stream, NC_KC_ELEM, 0.0, bytes);
        hipLaunchKernelGGL(encodec_stream_gather_kernel, dim3(gx, (unsigned)cnt), dim3(256), 0, m.stream, druns + done, carry.as<float>(), pcm, arena.as<float>(),
                           carry.as<float>());
        NC_HIP(hipGetLastError());
    });
    if (P.batches.empty()) return;   // nothing was completed: no model kernel
    m.run_batches(er_assign_lanes(P.rows, P.batches), true, [&](size_t i) {
        const ErBatch& bt = P.batches[i];
        const int N = (int)bt.count;
        const int64_t L = bt.key, Tz = P.rows[bt.first].frames;
        size_t li = first_launch[i];
        int64_t* cb = reinterpret_cast<int64_t*>(m.alloc((size_t)N * nqe * Tz * 2));
        float* sc = m.cfg.normalize ? m.alloc((size_t)N) : nullptr;
        float* eb = emb ? m.alloc((size_t)N * D * Tz) : nullptr;
        m.encode_batch(arena.as<float>() + x_off[i], N, L, Tz, cb, sc, eb);
        rg_copy_i64(m, t, li++, cb, codes);
        if (want_sc) rg_copy_f32(m, t, li++, sc, scales);
        if (emb) rg_copy_f32(m, t, li++, eb, emb);
    });
}

// ===================================================================================================================== Decode
void nc_encodec_stream_pool::decode_dev(EncodecModel& m, const EsPlan& P, const int64_t* codes, const float* scales, float* pcm) {
    const int C = m.cfg.channels;
    const int64_t n_rows = (int64_t)P.rows.size(), stride = g.stride;
    if (m.cfg.normalize && !scales && n_rows) fail(NC_EINVAL, "this model normalises frames: scales must be given");
    RgTables t;
    std::vector<size_t> first_launch;
    std::vector<int64_t> a_off;                     // of every batch's [N, C, Lo] output in the arena, behind the carry halves
    int64_t a_total = round_up(halves.elems(), kAlign);
    for (const ErBatch& bt : P.batches) {
        const int64_t N = (int64_t)bt.count, Tz = bt.key;
        first_launch.push_back(t.launches.size());
        t.begin(nq * P.total_frames, N * nq * Tz);
        for (int64_t r = 0; r < N; ++r) {
            const ErRow& w = P.rows[bt.first + (size_t)r];
            const EsEntry& e = P.e[(size_t)w.clip];
            t.add(nq * (e.in_off + e.before[(size_t)(w.seg - e.T0)]), r * nq * Tz, nq * Tz);
        }
        t.end();
        if (m.cfg.normalize) {
            t.begin(n_rows, N);
            for (int64_t r = 0; r < N; ++r) {
                const ErRow& w = P.rows[bt.first + (size_t)r];
                t.add(P.e[(size_t)w.clip].row_off + (w.seg - P.e[(size_t)w.clip].T0), r, 1);
            }
            t.end();
        }
        a_off.push_back(a_total);
        a_total += round_up(N * C * P.rows[bt.first].len, kAlign);
    }
    // the frame lists: per emitting entry the carried frame (if the stream has one) and this step's frames
    std::vector<OlaFrame> ftab;
    std::vector<EsOla> jobs;
    int64_t longest = 1;
    for (const EsEntry& e : P.e) {
        if (e.n_samples <= 0 && e.n_in == 0) continue;
        const Slot& s = slots[(size_t)e.id];
        const bool carried = e.T0 > 0;
        const int64_t first = (int64_t)ftab.size();
        std::vector<int64_t> flen;
        if (carried) {   // rows [C][ov] of the slot's current half stand for samples [stride, L_full) of the last full frame
            ftab.push_back({halves.at(s.cur, e.id) - stride, g.L_full, g.ov});
            flen.push_back(g.L_full);
        }
        int64_t last_off = -1;
        for (size_t r = 0; r < e.flen.size(); ++r) {
            const int bi = e.at[r].first, row = e.at[r].second;
            if (bi < 0) fail(NC_ESTATE, "internal: slot %d: a frame without a batch", e.id);
            const int64_t Lo = P.rows[P.batches[(size_t)bi].first].len, off = a_off[(size_t)bi] + (int64_t)row * C * Lo;
            if (off < round_up(halves.elems(), kAlign) || off + C * Lo > a_total) fail(NC_ESTATE, "internal: slot %d: a frame leaves the arena", e.id);
            ftab.push_back({off, Lo, Lo});
            flen.push_back(Lo);
            last_off = off;
        }
        const int nfr = (int)flen.size();
        const int64_t L0 = flen[0], t0 = carried ? stride : 0;
        const int64_t total = e.flush ? (int64_t)(nfr - 1) * stride + flen[(size_t)nfr - 1] : t0 + e.n_in * stride;
        if (total - t0 != e.n_samples) fail(NC_ESTATE, "internal: slot %d overlap-adds to %lld samples, planned %lld", e.id, (long long)(total - t0), (long long)e.n_samples);
        for (int f = 0; f < nfr; ++f)
            if (flen[(size_t)f] > L0 || (f + 1 < nfr && flen[(size_t)f] < stride)) fail(NC_EINVAL, "slot %d: frames that leave a gap or outgrow the first one", e.id);
        // a stream that emitted before its flush, or that holds a full frame, has the full window: no weight sum is <= 1e-10f (ola_eps,
        // L_full <= 2^25 at create).  A stream that begins and ends in this flush has the window of its own first frame: as the ragged call.
        const float eps = L0 == g.L_full ? 0.0f : ola_eps(flen, stride, total);
        const bool keeps = !e.flush && e.n_in > 0;   // the last frame is full: its tail is the slot's next carry
        for (int c = 0; c < C; ++c) {
            EsOla j{};
            j.clip = {C * e.out_off + c * e.n_samples, total, first, L0, nfr, c, eps, 0};
            j.t0 = t0;
            if (keeps) { j.carry_dst = halves.at(s.cur ^ 1, e.id) + (int64_t)c * g.ov; j.carry_src = last_off + (int64_t)c * g.L_full + stride; j.carry_n = g.ov; }
            if (j.clip.out < 0 || j.clip.out + e.n_samples > C * P.total_samples || (keeps && (j.carry_src + j.carry_n > a_total || j.carry_dst + j.carry_n > halves.elems())))
                fail(NC_ESTATE, "internal: slot %d: an overlap-add job leaves its tensors", e.id);
            jobs.push_back(j);
        }
        longest = std::max(longest, std::max(e.n_samples, g.ov));
    }
    if (jobs.empty()) return;
    t.extra.resize(jobs.size() * sizeof(EsOla) + ftab.size() * sizeof(OlaFrame));
    std::memcpy(t.extra.data(), jobs.data(), jobs.size() * sizeof(EsOla));
    std::memcpy(t.extra.data() + jobs.size() * sizeof(EsOla), ftab.data(), ftab.size() * sizeof(OlaFrame));
    grow_arena(m, a_total);
    LaneScope lanes(m);
    const char* extra = rg_upload(m, t);
    if (!P.batches.empty())
        m.run_batches(er_assign_lanes(P.rows, P.batches), true, [&](size_t i) {
            const ErBatch& bt = P.batches[i];
            const int N = (int)bt.count;
            const int64_t Tz = bt.key, Lo = P.rows[bt.first].len;
            size_t li = first_launch[i];
            int64_t* cb = reinterpret_cast<int64_t*>(m.alloc((size_t)N * nq * Tz * 2));
            float* sc = m.cfg.normalize ? m.alloc((size_t)N) : nullptr;
            rg_copy_i64(m, t, li++, codes, cb);
            if (sc) rg_copy_f32(m, t, li++, scales, sc);
            int64_t got = 0;
            const float* out = m.decode_batch(cb, N, nq, Tz, sc, &got);
            if (got != Lo) fail(NC_ESTATE, "internal: decoder produced %lld samples, planned %lld", (long long)got, (long long)Lo);
            NC_HIP(hipMemcpyAsync(arena.as<float>() + a_off[i], out, (size_t)N * C * Lo * 4, hipMemcpyDeviceToDevice, m.stream));
        });
    const EsOla* dj = reinterpret_cast<const EsOla*>(extra);
    const OlaFrame* dft = reinterpret_cast<const OlaFrame*>(extra + jobs.size() * sizeof(EsOla));
    const unsigned gx = copy_grid_x(longest, 4);
    for_grid_y(jobs.size(), [&](size_t done, size_t cnt) {
        ProfScope ps(&m.prof, m.stream, NC_KC_ELEM, 0.0, 8.0 * (double)C * (double)P.total_samples);
        hipLaunchKernelGGL(overlap_add_stream_kernel, dim3(gx, (unsigned)cnt), dim3(256), 0, m.stream, dj + done, dft, arena.as<float>(), stride, pcm);
        NC_HIP(hipGetLastError());
    });
}

// ================================================================================================ C ABI
namespace {

// elements of out_packed the step writes
int64_t out_elems(const nc_encodec_stream_pool& x, const EsPlan& P) {
    return x.decode ? (int64_t)x.model().cfg.channels * P.total_samples : (int64_t)x.model().n_q * P.total_frames;
}

void pool_step(nc_encodec_stream_pool& x, bool host, int32_t n, const int32_t* slots, const int64_t* n_in, const int32_t* flush, const int64_t* frame_lens,
               const void* in, const float* scales_in, void* out, float* scales_out, float* emb, int64_t out_cap, int32_t* n_frames, int64_t* n_out) {
    const char* what = host ? "nc_encodec_stream_pool_step" : "nc_encodec_stream_pool_step_dev";
    EncodecModel& m = x.model();
    const EsPlan P = x.plan(n, slots, n_in, flush, frame_lens, what);
    x.check(P);
    const int64_t need = out_elems(x, P);
    if (out_cap < need) fail(NC_EINVAL, "%s: out_cap is %lld, the step writes %lld elements (nc_encodec_stream_pool_query)", what, (long long)out_cap, (long long)need);
    if ((P.total_in > 0 && !in) || (need > 0 && !out)) fail(NC_EINVAL, "%s: null pointer", what);
    if (x.decode && m.cfg.normalize && !scales_in && !P.rows.empty()) fail(NC_EINVAL, "%s: this model normalises frames: scales must be given", what);
    if (!host) {
        x.step_dev(P, in, scales_in, out, scales_out, emb);
    } else {
        // The device part runs through encodec_host_run: a step changes no slot before it is through and writes only the halves of the
        // carry that the slots do not hold yet, so running it twice after a persistent-LSTM timeout is running it once.
        const size_t n_rows = P.rows.size();
        OwnStreamScope own(m);
        if (x.decode) {
            if (scales_in) h2d(x.sc_stage, scales_in, n_rows * 4, m.stream);
            pool_step_staged(x, m.stream, in, (size_t)x.nq * P.total_in * 8, out, (size_t)need * 4, nullptr, 0, [&](void* din, void* dout, float*) {
                encodec_host_run(m, [&] { x.step_dev(P, din, scales_in ? x.sc_stage.as<float>() : nullptr, dout, nullptr, nullptr); });
            });
        } else {
            x.sc_out.reserve(std::max<size_t>(n_rows * 4, 16));
            pool_step_staged(x, m.stream, in, (size_t)P.total_in * 4, out, (size_t)need * 8, emb, (size_t)m.cfg.dimension * P.total_frames * 4,
                             [&](void* din, void* dout, float* demb) {
                                 encodec_host_run(m, [&] { x.step_dev(P, din, nullptr, dout, x.sc_out.as<float>(), demb); });
                                 if (scales_out && m.cfg.normalize && n_rows) NC_HIP(hipMemcpyAsync(scales_out, x.sc_out.p, n_rows * 4, hipMemcpyDeviceToHost, m.stream));
                             });
        }
    }
    x.commit(P);
    for (size_t i = 0; i < P.e.size(); ++i) {
        if (n_frames) n_frames[i] = P.e[i].n_rows;
        if (n_out) n_out[i] = x.decode ? P.e[i].n_samples : P.e[i].code_frames;
    }
}

}  // namespace

extern "C" {

nc_status nc_encodec_stream_plan(const nc_encodec_config* cfg, int32_t decode, int32_t n, const int64_t* pushed, const int64_t* emitted, const int64_t* n_in,
                                 const int32_t* flush, const int64_t* frame_lens, int32_t max_rows, nc_encodec_ragged_plan* out, nc_encodec_ragged_row* rows,
                                 int64_t cap, int32_t* n_frames, int64_t* code_frames, int64_t* n_samples) {
    return guard([&] {
        const char* what = "nc_encodec_stream_plan";
        if (!cfg) fail(NC_EINVAL, "cfg must not be null");
        const EncodecModel m(*cfg);   // host arithmetic alone: no device is touched
        const EsGeom g = geom_of(m, what);
        if (!pushed || !emitted || !n_in) fail(NC_EINVAL, "%s: null pointer", what);
        if (n <= 0) fail(NC_EINVAL, "%s: n must be positive", what);
        std::vector<int64_t> next0((size_t)n, 0);
        for (int i = 0; i < n; ++i) {   // the position of a stream that has not been flushed follows from what it has received
            if (pushed[i] < 0) fail(NC_EINVAL, "%s: stream %d: pushed is negative", what, i);
            const int64_t want = decode ? pushed[i] * g.stride : (pushed[i] >= g.seg ? (pushed[i] - g.seg) / g.stride + 1 : 0);
            if (emitted[i] != want)
                fail(NC_EINVAL, "%s: stream %d: a stream that has received %lld has emitted %lld, not %lld", what, i, (long long)pushed[i], (long long)want, (long long)emitted[i]);
            next0[(size_t)i] = decode ? 0 : want;
        }
        report(m, m.n_q, make_plan(m, g, decode != 0, n, nullptr, pushed, next0.data(), n_in, flush, frame_lens, max_rows, what), out, rows, cap, n_frames,
               code_frames, n_samples);
    });
}

nc_status nc_encodec_stream_pool_create(nc_codec* h, int32_t decode, int32_t n_slots, int32_t n_q, nc_encodec_stream_pool** out) {
    return guard([&] {
        if (!out) fail(NC_EINVAL, "out must not be null");
        *out = nullptr;
        EncodecModel& m = as<EncodecModel>(h);
        std::unique_ptr<nc_encodec_stream_pool> p(new nc_encodec_stream_pool);
        p->h = h;
        p->decode = decode != 0;
        p->g = geom_of(m, "nc_encodec_stream_pool_create");
        if (n_slots <= 0 || n_slots > 65536) fail(NC_EINVAL, "n_slots must be in 1..65536");
        if (n_q < 0 || n_q > m.cfg.n_codebooks) fail(NC_EINVAL, "codes carry %d codebooks; the model has %d", n_q, m.cfg.n_codebooks);
        p->nq = n_q > 0 ? n_q : m.n_q;
        p->slots.resize((size_t)n_slots);
        p->halves = {n_slots, round_up((int64_t)m.cfg.channels * (p->decode ? p->g.ov : p->g.seg), 4)};
        m.use_device();
        if (p->decode) p->arena.reserve((size_t)(round_up(p->halves.elems(), kAlign) + (int64_t)n_slots * m.cfg.channels * p->g.L_full) * 4);
        else p->carry.reserve((size_t)p->halves.elems() * 4);
        *out = p.release();
    });
}

nc_status nc_encodec_stream_pool_destroy(nc_encodec_stream_pool* p) {
    return guard([&] { delete p; });
}

nc_status nc_encodec_stream_pool_reset_slot(nc_encodec_stream_pool* p, int32_t slot) {
    return guard([&] {
        reset_keep_cur(slot_of(pool_of(p), slot));
    });
}

nc_status nc_encodec_stream_pool_pending(const nc_encodec_stream_pool* p, int32_t slot, int64_t* n) {
    return guard([&] {
        if (!n) fail(NC_EINVAL, "n must not be null");
        nc_encodec_stream_pool& x = pool_of(p);
        const nc_encodec_stream_pool::Slot& s = slot_of(x, slot);
        if (s.ended) *n = 0;
        else if (x.decode) *n = s.T > 0 ? x.g.ov : 0;
        else *n = s.T - s.next * x.g.stride;
    });
}

nc_status nc_encodec_stream_pool_query(const nc_encodec_stream_pool* p, int32_t n, const int32_t* slots, const int64_t* n_in, const int32_t* flush,
                                       const int64_t* frame_lens, int32_t* n_frames, int64_t* code_frames, int64_t* n_samples) {
    return guard([&] {
        nc_encodec_stream_pool& x = pool_of(p);
        const EsPlan P = x.plan(n, slots, n_in, flush, frame_lens, "nc_encodec_stream_pool_query");
        report(x.model(), x.decode ? x.nq : x.model().n_q, P, nullptr, nullptr, 0, n_frames, code_frames, n_samples);
    });
}

nc_status nc_encodec_stream_pool_plan(const nc_encodec_stream_pool* p, int32_t n, const int32_t* slots, const int64_t* n_in, const int32_t* flush,
                                      const int64_t* frame_lens, nc_encodec_ragged_plan* out, nc_encodec_ragged_row* rows, int64_t cap) {
    return guard([&] {
        nc_encodec_stream_pool& x = pool_of(p);
        if (!out) fail(NC_EINVAL, "out must not be null");
        const EsPlan P = x.plan(n, slots, n_in, flush, frame_lens, "nc_encodec_stream_pool_plan");
        report(x.model(), x.decode ? x.nq : x.model().n_q, P, out, rows, cap, nullptr, nullptr, nullptr);
    });
}

nc_status nc_encodec_stream_pool_step(nc_encodec_stream_pool* p, int32_t n, const int32_t* slots, const int64_t* n_in, const int32_t* flush,
                                      const int64_t* frame_lens, const void* in_packed, const float* scales_in, void* out_packed, float* scales_out,
                                      float* emb_packed, int64_t out_cap, int32_t* n_frames, int64_t* n_out) {
    return guard([&] { pool_step(pool_of(p), true, n, slots, n_in, flush, frame_lens, in_packed, scales_in, out_packed, scales_out, emb_packed, out_cap, n_frames, n_out); });
}

nc_status nc_encodec_stream_pool_step_dev(nc_encodec_stream_pool* p, int32_t n, const int32_t* slots, const int64_t* n_in, const int32_t* flush,
                                          const int64_t* frame_lens, const void* in_packed, const float* scales_in, void* out_packed, float* scales_out,
                                          float* emb_packed, int64_t out_cap, int32_t* n_frames, int64_t* n_out) {
    return guard([&] { pool_step(pool_of(p), false, n, slots, n_in, flush, frame_lens, in_packed, scales_in, out_packed, scales_out, emb_packed, out_cap, n_frames, n_out); });
}

}  // extern "C"
