// What incremental sessions (nc_session.hip) and the session pool (nc_session_pool.hip) share: the schedule of one stream, the row
// families of its tensors and the frame arithmetic of one step.  The device-side copy of a concatenation that
// their kernels are made of is concat_copy (nc_copy.h).
#pragma once
#include <algorithm>

#include "nc_copy.h"
#include "nc_guard.h"

namespace nc {

constexpr int SS_MAX_LEVELS = 8;

inline int64_t ss_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- schedule --------------------------------------------------------------------------------------------------------------------
struct SsStep { int64_t w0, w1, k0, k1, h0n; };   // window, kept frames, first resident frame afterwards

inline SsStep step_push(int64_t hl, int64_t hr, int64_t align, int64_t E, int64_t P1) {
    const int64_t h0 = std::max<int64_t>(0, E - hl), e1 = P1 > hr ? (P1 - hr) / align * align : 0;
    SsStep s;
    s.k0 = E; s.k1 = std::max(E, e1);
    s.w0 = h0; s.w1 = s.k1 > s.k0 ? P1 : h0;
    s.h0n = std::max<int64_t>(0, s.k1 - hl);
    return s;
}
inline SsStep step_flush(int64_t hl, int64_t E, int64_t P1) { return {std::max<int64_t>(0, E - hl), P1, E, P1, P1}; }

inline void session_halos(const nc_halo& h, bool decode, int64_t& hl, int64_t& hr) {   // as make_plan (nc_chunk.hip)
    hl = decode ? h.dec_right : h.enc_right;
    hr = decode ? h.dec_left : h.enc_left;
    if (h.align <= 0 || hl < 0 || hr < 0 || hl % h.align != 0 || hr % h.align != 0) fail(NC_EINVAL, "halo: align must be positive and divide the halos");
}

inline uint64_t mix_seed(uint64_t seed, int64_t frame) { return seed ^ (0x9E3779B97F4A7C15ull * ((uint64_t)frame + 1)); }

// ---- row families ----------------------------------------------------------------------------------------------------------------
// Level i of a family holds u * mul[i] / div[i] elements per row for u units (frames; samples for the PCM).  Caller-side tensors and the
// window keep the levels of a row side by side (row_major: SNAC codes) or level after level (DAC codes, PCM, noise stages); the history
// is always level after level with dense rows.
struct Family {
    int nl = 1;
    int64_t mul[SS_MAX_LEVELS] = {1}, div[SS_MAX_LEVELS] = {1};
    bool row_major = false;
    int64_t len(int i, int64_t u) const { return u * mul[i] / div[i]; }
    int64_t total(int64_t u) const {
        int64_t n = 0;
        for (int i = 0; i < nl; ++i) n += len(i, u);
        return n;
    }
};
struct Lay { int64_t len[SS_MAX_LEVELS], base[SS_MAX_LEVELS], pitch[SS_MAX_LEVELS]; };
inline Lay lay_of(const Family& f, int64_t u, int64_t rows, bool row_major) {
    Lay l{};
    int64_t off = 0;
    for (int i = 0; i < f.nl; ++i) {
        l.len[i] = f.len(i, u);
        l.base[i] = row_major ? off : rows * off;
        l.pitch[i] = row_major ? f.total(u) : l.len[i];
        off += l.len[i];
    }
    return l;
}

// ---- one stream --------------------------------------------------------------------------------------------------------------------
// What a stream is on its handle: direction, halos, rates and row families.  B rows move in lockstep (a pool slot: B = 1).
struct SessionGeom {
    nc_codec* h = nullptr;
    bool dac = true, decode = true, with_noise = false;
    int B = 1, nq = 0, n_codebooks = 0;
    int64_t hl = 0, hr = 0, align = 1;
    int64_t hop = 1;              // input samples per frame (encode)
    int64_t H = 1;                // output samples per frame (decode)
    Family codes;                 // the code levels (SNAC) / the one code row family (DAC), in frames
    Family main, noise;           // what is pushed: the codes (decode) or the PCM (encode); the NoiseBlock inputs

    int rows() const { return dac && decode ? B * nq : B; }
    int out_rows() const { return !decode && dac ? B * n_codebooks : B; }
    size_t elt() const { return decode ? 8 : 4; }
    int64_t unit() const { return hop * align; }
    // frames a push of n_in (0: the flush) can emit at most, whatever the state
    int64_t cap_frames(int64_t n_in) const {
        if (decode) return n_in > 0 ? n_in : hr + align;
        return n_in > 0 ? (n_in / unit() + 1) * align : hr + 2 * align;
    }
    int64_t out_elems(int64_t frames) const {   // per row
        if (decode) return frames * H;
        return codes.total(frames);   // DAC: per codebook row; SNAC: all levels of a row
    }
};
// fills g from a DAC or SNAC handle (NC_EUNSUPPORTED for Encodec, NC_EINVAL for B <= 0, a bad n_q or rows beyond one launch grid)
void session_geom(nc_codec* h, bool decode, int B, int n_q, SessionGeom& g);

// frames pushed and emitted, samples pushed (encode), first resident frame, which history buffer is current
struct SessionState {
    int64_t P = 0, E = 0, S = 0, h0 = 0;
    bool flushed = false;
    int cur = 0;
};

// One step on frame counts alone: a push of n_in units or the flush.  Nothing here touches the device or the state.
struct SessionMove {
    SsStep st;
    int64_t P1, S1;
    bool run;                                   // the step runs a window
    int64_t Wf, ke, k_off;                      // window width, kept frames, first kept frame inside the window
    int64_t hist_u, new_u, win_u, next_off_u, next_u;   // units: frames (decode) or samples (encode)
    int64_t nout, Lw;                           // outputs per row; decoded samples per window row
};
// NC_EINVAL where the state refuses the step: after a flush, n_in outside 1..2^30, a misaligned decode push, a flush of nothing
void session_check(const SessionGeom& g, const SessionState& s, int64_t n_in, bool flush);
SessionMove session_move(const SessionGeom& g, const SessionState& s, int64_t n_in, bool flush);
inline void session_commit(SessionState& s, const SessionMove& mv, bool flush) {
    s.P = mv.P1; s.S = mv.S1; s.E = mv.st.k1; s.h0 = mv.st.h0n; s.cur = 1 - s.cur;
    s.flushed = flush;
}

}  // namespace nc
