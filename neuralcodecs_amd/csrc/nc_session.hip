// Incremental sessions: DAC / SNAC codes or PCM pushed as they arrive (include/nc_mi355x.h, "incremental sessions").
//
// Schedule.  P frames pushed, E emitted, hl / hr the halos of the direction as make_plan of nc_chunk.hip assigns them.  The resident
// history is [h0, P) with h0 = max(0, E - hl) at all times.  A push of n frames makes P' = P + n and e' = floor_align(P' - hr); when
// e' > E the step runs the window [h0, P') -- the history followed by the pushed frames, nothing else -- through the EXISTING launch
// sequence, keeps [E, e') and advances E.  The flush runs [h0, P) and keeps [E, P).  Invariants: E >= floor_align(P - hr) after every
// push, so P - E < hr + align and the history holds at most hl + hr + align frames; a kept frame is at least hl behind the window's
// left edge unless that edge is frame 0 (the clip's true start) and at least hr in front of its right edge unless the step is the flush
// (the clip's true end).  That is the premise of the chunked calls (nc_chunk.hip), so every kept output is the one-shot number.
//
// The schedule, the row families and the frame arithmetic of a step live in nc_session.h, shared with the session pool.
//
// Device work.  Two kernels, no tables: their few row families travel as kernel arguments.
//   session_assemble  one launch builds the window rows as history followed by the pushed data (followed by +0.0f where an encode flush
//                     pads the last hop) AND writes the next history, a suffix of the same concatenation, into the session's other
//                     history buffer (the two alternate, so no launch reads what it writes).
//   session_emit      one launch copies the kept columns of the window's output into the caller's rows.
// Both write with 16-byte stores from the first 16-byte boundary of a destination row, a scalar head in front and a scalar tail behind
// (the idiom of ragged_gather_* / ragged_scatter_*).  Everything else a step launches is the *_dev launch sequence on the handle's
// ck_* buffers; a process that creates no session launches what it launched before.
#include "nc_session.h"

namespace nc {

namespace {

// ---- kernels ---------------------------------------------------------------------------------------------------------------------
// (concat_copy, the copy both kernels are made of: nc_copy.h)
// One row family of an assembly launch (a code level, a noise stage, the PCM): `rows` rows, each hist_n resident elements followed by
// new_n pushed ones.  The window row takes the first win_n elements of that concatenation (+0 behind its end); the next history is
// its elements [next_off, hist_n + new_n).  History rows are dense; the pushed data and the window have a base and a row pitch.
struct SsLevel {
    int64_t hist_n, new_n, win_n, next_off;
    int64_t hist_base, new_base, new_pitch, win_base, win_pitch, next_base;
};
struct SsArgs {
    int32_t n_levels, rows;
    SsLevel lv[SS_MAX_LEVELS];
};
// blockIdx.y = row, blockIdx.z = 2 * level + (0: window, 1: next history), blockIdx.x strides over the row
template <class T>
__device__ __forceinline__ void assemble_body(const SsArgs& a, const T* __restrict__ hist, const T* __restrict__ nw, T* __restrict__ win,
                                              T* __restrict__ next) {
    const SsLevel& L = a.lv[blockIdx.z >> 1];
    const int64_t row = blockIdx.y;
    const T* h = hist + L.hist_base + row * L.hist_n;
    const T* n = nw + L.new_base + row * L.new_pitch;
    if ((blockIdx.z & 1) == 0) {
        if (win && L.win_n > 0) concat_copy<T>(h, L.hist_n, n, L.new_n, 0, win + L.win_base + row * L.win_pitch, L.win_n);
    } else {
        const int64_t next_n = L.hist_n + L.new_n - L.next_off;
        if (next_n > 0) concat_copy<T>(h, L.hist_n, n, L.new_n, L.next_off, next + L.next_base + row * next_n, next_n);
    }
}
__global__ __launch_bounds__(256) void session_assemble_f32(SsArgs a, const float* __restrict__ hist, const float* __restrict__ nw,
                                                            float* __restrict__ win, float* __restrict__ next) {
    assemble_body<float>(a, hist, nw, win, next);
}
__global__ __launch_bounds__(256) void session_assemble_i64(SsArgs a, const int64_t* __restrict__ hist, const int64_t* __restrict__ nw,
                                                            int64_t* __restrict__ win, int64_t* __restrict__ next) {
    assemble_body<int64_t>(a, hist, nw, win, next);
}

// kept columns: n elements from src_base + row * src_pitch to dst_base + row * dst_pitch.  blockIdx.y = row, blockIdx.z = level
struct SsEmitLevel { int64_t n, src_base, src_pitch, dst_base, dst_pitch; };
struct SsEmitArgs {
    int32_t n_levels, rows;
    SsEmitLevel lv[SS_MAX_LEVELS];
};
template <class T>
__device__ __forceinline__ void emit_body(const SsEmitArgs& a, const T* __restrict__ src, T* __restrict__ dst) {
    const SsEmitLevel& L = a.lv[blockIdx.z];
    const int64_t row = blockIdx.y;
    if (L.n > 0) concat_copy<T>(src + L.src_base + row * L.src_pitch, L.n, nullptr, 0, 0, dst + L.dst_base + row * L.dst_pitch, L.n);
}
__global__ __launch_bounds__(256) void session_emit_f32(SsEmitArgs a, const float* __restrict__ src, float* __restrict__ dst) {
    emit_body<float>(a, src, dst);
}
__global__ __launch_bounds__(256) void session_emit_i64(SsEmitArgs a, const int64_t* __restrict__ src, int64_t* __restrict__ dst) {
    emit_body<int64_t>(a, src, dst);
}

// ---- launches (schedule and row families: nc_session.h) ---------------------------------------------------------------------------
// hist (hist_u units per row) ++ nw (new_u) -> win (win_u units per row; null: no window) and next (the units from next_off_u on)
template <class T>
void assemble(Codec& m, void (*kernel)(SsArgs, const T*, const T*, T*, T*), const Family& f, int rows, int64_t hist_u, int64_t new_u,
              int64_t win_u, int64_t next_off_u, const T* hist, const T* nw, T* win, T* next) {
    const int64_t next_u = hist_u + new_u - next_off_u;
    if (next_u < 0 || next_off_u < 0) fail(NC_ESTATE, "internal: session history of %lld units", (long long)next_u);
    const Lay lh = lay_of(f, hist_u, rows, false), ln = lay_of(f, new_u, rows, f.row_major), lw = lay_of(f, win_u, rows, f.row_major),
              lx = lay_of(f, next_u, rows, false);
    SsArgs a{};
    a.n_levels = f.nl; a.rows = rows;
    int64_t longest = 0;
    double bytes = 0;
    for (int i = 0; i < f.nl; ++i) {
        SsLevel& L = a.lv[i];
        L.hist_n = lh.len[i]; L.new_n = ln.len[i]; L.win_n = win ? lw.len[i] : 0; L.next_off = lh.len[i] + ln.len[i] - lx.len[i];
        L.hist_base = lh.base[i]; L.new_base = ln.base[i]; L.new_pitch = ln.pitch[i];
        L.win_base = lw.base[i]; L.win_pitch = lw.pitch[i]; L.next_base = lx.base[i];
        if (L.next_off < 0) fail(NC_ESTATE, "internal: session history offset");
        longest = std::max(longest, std::max(L.win_n, lx.len[i]));
        bytes += (double)rows * 2.0 * (double)(L.win_n + lx.len[i]) * sizeof(T);
    }
    if (longest <= 0) return;
    ProfScope ps(&m.prof, m.stream, NC_KC_ELEM, 0.0, bytes);
    hipLaunchKernelGGL(kernel, dim3(copy_grid_x(longest, sizeof(T)), (unsigned)rows, (unsigned)(2 * f.nl)), dim3(256), 0, m.stream, a, hist, nw, win, next);
    NC_HIP(hipGetLastError());
}

template <class T>
void emit(Codec& m, void (*kernel)(SsEmitArgs, const T*, T*), int nl, int rows, const SsEmitLevel* lv, const T* src, T* dst) {
    SsEmitArgs a{};
    a.n_levels = nl; a.rows = rows;
    int64_t longest = 0;
    double bytes = 0;
    for (int i = 0; i < nl; ++i) {
        a.lv[i] = lv[i];
        longest = std::max(longest, lv[i].n);
        bytes += (double)rows * 2.0 * (double)lv[i].n * sizeof(T);
    }
    if (longest <= 0) return;
    ProfScope ps(&m.prof, m.stream, NC_KC_ELEM, 0.0, bytes);
    hipLaunchKernelGGL(kernel, dim3(copy_grid_x(longest, sizeof(T)), (unsigned)rows, (unsigned)nl), dim3(256), 0, m.stream, a, src, dst);
    NC_HIP(hipGetLastError());
}

}  // namespace

}  // namespace nc

using namespace nc;

// the opaque session of the C ABI: what the stream is (SessionGeom), where it stands (SessionState), and its device buffers
struct nc_session : SessionGeom, SessionState {
    uint64_t seed = 0;
    DevBuf hist[2], nhist[2];     // resident history of the main tensor and of the noise, alternating
    DevBuf in_stage, nz_stage, out_stage;   // host-pointer calls and drawn noise
};

namespace nc {

void session_check(const SessionGeom& g, const SessionState& s, int64_t n_in, bool flush) {
    if (s.flushed) fail(NC_EINVAL, "the session has been flushed: nc_session_reset starts the next clip");
    if (!flush) {
        if (n_in <= 0 || n_in > ((int64_t)1 << 30)) fail(NC_EINVAL, "n_in must be in 1..2^30");
        if (g.decode && n_in % g.align != 0) fail(NC_EINVAL, "a push of %lld frames is not a multiple of %lld", (long long)n_in, (long long)g.align);
    } else if ((g.decode ? s.P : s.S) <= 0) {
        fail(NC_EINVAL, "nothing has been pushed");
    }
}

void session_geom(nc_codec* h, bool decode, int B, int n_q, SessionGeom& g) {
    codec_of(h);
    if (h->kind == EncodecModel::kKind) fail(NC_EUNSUPPORTED, "Encodec handles have no sessions: 48 kHz is segmented per second already, the 24 kHz LSTM has unbounded context");
    if (B <= 0 || n_q < 0) fail(NC_EINVAL, "B must be positive and n_q must not be negative");
    g.h = h; g.dac = h->kind == DacModel::kKind; g.decode = decode; g.B = B;
    nc_halo halo{};
    int nd = 0;
    const int32_t* dr = nullptr;
    if (g.dac) {
        const DacModel& m = as<DacModel>(h);
        if (n_q > m.cfg.n_codebooks) fail(NC_EINVAL, "n_q = %d exceeds the model's %d codebooks", n_q, m.cfg.n_codebooks);
        if (nc_dac_halo(&m.cfg, &halo) != NC_OK) fail(NC_EINVAL, "%s", get_last_error());
        g.n_codebooks = m.cfg.n_codebooks;
        g.nq = n_q > 0 ? n_q : m.cfg.n_codebooks;
        g.hop = m.hop;
        nd = m.cfg.n_decoder_rates; dr = m.cfg.decoder_rates;
        g.codes.row_major = false;   // [B, n_q, frames]: one family of B * n_q rows
    } else {
        const SnacModel& m = as<SnacModel>(h);
        if (nc_snac_halo(&m.cfg, &halo) != NC_OK) fail(NC_EINVAL, "%s", get_last_error());
        if (m.pad_to != (int64_t)m.hop * halo.align) fail(NC_ESTATE, "internal: SNAC pads to %lld samples, the halo aligns to %lld frames", (long long)m.pad_to, (long long)halo.align);
        g.hop = m.hop;
        nd = m.cfg.n_decoder_rates; dr = m.cfg.decoder_rates;
        g.with_noise = g.decode && m.cfg.noise != 0;
        g.codes.nl = m.cfg.n_vq_strides;
        for (int i = 0; i < g.codes.nl; ++i) { g.codes.mul[i] = 1; g.codes.div[i] = m.cfg.vq_strides[i]; }
        g.codes.row_major = true;    // the levels of a row side by side
        g.noise.nl = nd;
        int64_t S = 1;
        for (int i = 0; i < nd; ++i) { S *= dr[i]; g.noise.mul[i] = S; g.noise.div[i] = 1; }
    }
    for (int i = 0; i < nd; ++i) g.H *= dr[i];
    session_halos(halo, g.decode, g.hl, g.hr);
    g.align = halo.align;
    if (g.decode) g.main = g.codes;   // an encode session's main family is the PCM: one level of samples (the default Family)
    if ((int64_t)g.rows() > 65535 || (int64_t)B * std::max(1, g.n_codebooks) > 65535) fail(NC_EINVAL, "B = %d rows exceed one launch grid", B);
}

SessionMove session_move(const SessionGeom& g, const SessionState& s, int64_t n_in, bool flush) {
    Codec& m = codec_of(g.h);
    SessionMove v{};
    v.new_u = flush ? 0 : n_in;                                               // pushed units: frames (decode) or samples (encode)
    v.S1 = s.S + (g.decode ? 0 : v.new_u);
    if (g.decode) v.P1 = s.P + v.new_u;
    else v.P1 = flush ? ss_ceil_div(v.S1, g.unit()) * g.align : v.S1 / g.unit() * g.align;   // the flush pads as the codec's own Preprocess does
    v.st = flush ? step_flush(g.hl, s.E, v.P1) : step_push(g.hl, g.hr, g.align, s.E, v.P1);
    if (v.st.w0 != s.h0) fail(NC_ESTATE, "internal: session history starts at frame %lld, the window at %lld", (long long)s.h0, (long long)v.st.w0);
    v.run = v.st.k1 > v.st.k0;
    v.Wf = v.P1 - s.h0; v.ke = v.st.k1 - v.st.k0; v.k_off = v.st.k0 - s.h0;
    const int64_t per = g.decode ? 1 : g.hop;                                 // units per frame
    v.hist_u = (g.decode ? s.P : s.S) - s.h0 * per;
    v.win_u = v.run ? v.Wf * per : 0;
    v.next_off_u = std::min((v.st.h0n - s.h0) * per, v.hist_u + v.new_u);
    v.next_u = v.hist_u + v.new_u - v.next_off_u;
    if (v.run && g.decode) {
        v.Lw = g.dac ? static_cast<DacModel&>(m).decoded_len(v.Wf) : static_cast<SnacModel&>(m).decoded_len(v.Wf);
        v.nout = flush ? v.Lw - v.k_off * g.H : v.ke * g.H;
        if (v.nout <= 0 || v.k_off * g.H + v.nout > v.Lw) fail(NC_ESTATE, "internal: decoded window of %lld samples does not cover its kept frames", (long long)v.Lw);
    } else if (v.run) {
        v.nout = g.out_elems(v.ke);
    }
    return v;
}

}  // namespace nc

namespace {

void step(nc_session& s, bool host, const void* in, int64_t n_in, const float* noise, void* out, int64_t out_cap, int64_t* n_out, bool flush) {
    Codec& m = codec_of(s.h);
    if (!out || !n_out) fail(NC_EINVAL, "out and n_out must not be null");
    if (!flush && !in && !s.flushed) fail(NC_EINVAL, "in must not be null");
    session_check(s, s, n_in, flush);
    if (!m.loaded) fail(NC_ESTATE, "weights not loaded (call nc_codec_load_weights first)");
    if (out_cap < s.out_elems(s.cap_frames(flush ? 0 : n_in)))
        fail(NC_EINVAL, "out_cap %lld is below what nc_session_query asks for (%lld)", (long long)out_cap, (long long)s.out_elems(s.cap_frames(flush ? 0 : n_in)));

    // ---- the step, on frame counts alone
    const SessionMove mv = session_move(s, s, n_in, flush);
    const bool run = mv.run;
    const int64_t Wf = mv.Wf, ke = mv.ke, k_off = mv.k_off, hist_u = mv.hist_u, new_u = mv.new_u, win_u = mv.win_u, next_off_u = mv.next_off_u,
                  next_u = mv.next_u, nout = mv.nout, Lw = mv.Lw;
    const int rows = s.rows();
    if (nout > out_cap) fail(NC_ESTATE, "internal: a step of %lld outputs per row exceeds the queried capacity", (long long)nout);

    // ---- launches
    m.use_device();
    const int nxt = 1 - s.cur;
    const size_t elt = s.elt();
    const void* src = in;
    if (host && new_u > 0) {
        const size_t bytes = (size_t)rows * s.main.total(new_u) * elt;
        s.in_stage.reserve(bytes);
        NC_HIP(hipMemcpyAsync(s.in_stage.p, in, bytes, hipMemcpyHostToDevice, m.stream));
        src = s.in_stage.p;
    }
    s.hist[nxt].reserve(std::max<size_t>(16, (size_t)rows * s.main.total(next_u) * elt));
    if (s.decode) {
        int64_t* win = nullptr;
        if (run) {
            m.ck_codes.reserve((size_t)rows * s.main.total(Wf) * 8);
            win = m.ck_codes.as<int64_t>();
        }
        assemble<int64_t>(m, session_assemble_i64, s.main, rows, hist_u, new_u, win_u, next_off_u, s.hist[s.cur].as<int64_t>(),
                          static_cast<const int64_t*>(src), win, s.hist[nxt].as<int64_t>());
        float* nwin = nullptr;
        if (s.with_noise) {
            const float* nz = noise;
            if (new_u > 0) {
                const size_t bytes = (size_t)s.B * s.noise.total(new_u) * 4;
                if (!noise) {   // drawn per push from (seed, frame position)
                    s.nz_stage.reserve(bytes);
                    launch_randn(s.nz_stage.as<float>(), (int64_t)(bytes / 4), mix_seed(s.seed, s.P), m.stream);
                    nz = s.nz_stage.as<float>();
                } else if (host) {
                    s.nz_stage.reserve(bytes);
                    NC_HIP(hipMemcpyAsync(s.nz_stage.p, noise, bytes, hipMemcpyHostToDevice, m.stream));
                    nz = s.nz_stage.as<float>();
                }
            }
            s.nhist[nxt].reserve(std::max<size_t>(16, (size_t)s.B * s.noise.total(next_u) * 4));
            if (run) {
                m.ck_noise.reserve((size_t)s.B * s.noise.total(Wf) * 4);
                nwin = m.ck_noise.as<float>();
            }
            assemble<float>(m, session_assemble_f32, s.noise, s.B, hist_u, new_u, win_u, next_off_u, s.nhist[s.cur].as<float>(), nz, nwin,
                            s.nhist[nxt].as<float>());
        }
        if (run) {
            m.ck_out.reserve((size_t)s.B * Lw * 4);
            if (s.dac) {
                DacModel& d = static_cast<DacModel&>(m);
                m.ck_a.reserve((size_t)s.B * d.latent * Wf * 4);
                d.from_codes_dev(m.ck_codes.as<int64_t>(), s.B, s.nq, Wf, m.ck_a.as<float>());
                d.decode_dev(m.ck_a.as<float>(), s.B, Wf, m.ck_out.as<float>());
            } else {
                static_cast<SnacModel&>(m).decode_dev(m.ck_codes.as<int64_t>(), s.B, Wf, nwin, s.seed, m.ck_out.as<float>());
            }
            float* dst = static_cast<float*>(out);
            int64_t pitch = out_cap;
            if (host) {
                s.out_stage.reserve((size_t)s.B * nout * 4);
                dst = s.out_stage.as<float>();
                pitch = nout;
            }
            const SsEmitLevel lv{nout, k_off * s.H, Lw, 0, pitch};
            emit<float>(m, session_emit_f32, 1, s.B, &lv, m.ck_out.as<float>(), dst);
            if (host) m.copy2d(out, true, (size_t)out_cap * 4, dst, false, (size_t)nout * 4, (size_t)nout * 4, (size_t)s.B);
        }
    } else {
        float* win = nullptr;
        if (run) {
            m.ck_in.reserve((size_t)s.B * win_u * 4);
            win = m.ck_in.as<float>();
        }
        assemble<float>(m, session_assemble_f32, s.main, s.B, hist_u, new_u, win_u, next_off_u, s.hist[s.cur].as<float>(),
                        static_cast<const float*>(src), win, s.hist[nxt].as<float>());
        if (run) {
            const int64_t cw = s.codes.total(Wf);   // codes per row of the window: DAC per codebook, SNAC all levels
            const int crow = s.dac ? s.B * s.n_codebooks : s.B;
            m.ck_codes.reserve((size_t)crow * cw * 8);
            if (s.dac) static_cast<DacModel&>(m).encode_dev(win, s.B, win_u, 0, 0, m.ck_codes.as<int64_t>(), nullptr, nullptr);
            else static_cast<SnacModel&>(m).encode_dev(win, s.B, win_u, m.ck_codes.as<int64_t>(), nullptr, nullptr, true);
            int64_t* dst = static_cast<int64_t*>(out);
            int64_t pitch = out_cap;
            if (host) {
                s.out_stage.reserve((size_t)crow * nout * 8);
                dst = s.out_stage.as<int64_t>();
                pitch = nout;
            }
            const Lay lw = lay_of(s.codes, Wf, crow, s.codes.row_major), lk = lay_of(s.codes, ke, crow, true);
            SsEmitLevel lv[SS_MAX_LEVELS];
            for (int i = 0; i < s.codes.nl; ++i) lv[i] = {lk.len[i], lw.base[i] + s.codes.len(i, k_off), lw.pitch[i], lk.base[i], pitch};
            emit<int64_t>(m, session_emit_i64, s.codes.nl, crow, lv, m.ck_codes.as<int64_t>(), dst);
            if (host) m.copy2d(out, true, (size_t)out_cap * 8, dst, false, (size_t)nout * 8, (size_t)nout * 8, (size_t)crow);
        }
    }
    // ---- the session moves on only once everything is queued
    session_commit(s, mv, flush);
    *n_out = nout;
}

// A host-pointer call: on the handle's own stream, complete on return.
template <class F>
void host_call(nc_session* s, F&& f) {
    if (!s) fail(NC_EINVAL, "null session");
    Codec& m = codec_of(s->h);
    OwnStreamScope own(m);
    f();
    NC_HIP(hipStreamSynchronize(m.stream));
}

nc_session& session_of(const nc_session* s) {
    if (!s) fail(NC_EINVAL, "null session");
    return *const_cast<nc_session*>(s);
}

}  // namespace

// ================================================================================================ C ABI
extern "C" {

nc_status nc_session_schedule(const nc_halo* halo, int32_t decode, int32_t n_pushes, const int64_t* push_frames, int32_t flush,
                              nc_session_step* steps) {
    return guard([&] {
        if (!halo || !steps) fail(NC_EINVAL, "halo and steps must not be null");
        if (n_pushes < 0 || (n_pushes > 0 && !push_frames)) fail(NC_EINVAL, "n_pushes must not be negative and push_frames must not be null");
        if (n_pushes == 0) fail(NC_EINVAL, flush ? "nothing to flush" : "no pushes");
        int64_t hl, hr;
        session_halos(*halo, decode != 0, hl, hr);
        for (int i = 0; i < n_pushes; ++i)
            if (push_frames[i] <= 0 || push_frames[i] % halo->align != 0 || push_frames[i] > ((int64_t)1 << 40))
                fail(NC_EINVAL, "push %d: %lld frames is not a positive multiple of %lld", i, (long long)push_frames[i], (long long)halo->align);
        int64_t P = 0, E = 0;
        for (int i = 0; i < n_pushes + (flush ? 1 : 0); ++i) {
            const bool fl = i == n_pushes;
            if (!fl) P += push_frames[i];
            const SsStep st = fl ? step_flush(hl, E, P) : step_push(hl, hr, halo->align, E, P);
            steps[i] = {st.w0, st.w1, st.k0, st.k1, P - st.h0n};
            E = st.k1;
        }
    });
}

nc_status nc_session_create(nc_codec* h, int32_t decode, int32_t B, int32_t n_q, nc_session** out) {
    return guard([&] {
        if (!out) fail(NC_EINVAL, "out must not be null");
        *out = nullptr;
        std::unique_ptr<nc_session> s(new nc_session);
        session_geom(h, decode != 0, B, n_q, *s);
        *out = s.release();
    });
}

nc_status nc_session_destroy(nc_session* s) {
    return guard([&] { delete s; });
}

nc_status nc_session_reset(nc_session* s) {
    return guard([&] { static_cast<SessionState&>(session_of(s)) = SessionState{}; });
}

nc_status nc_session_set_seed(nc_session* s, uint64_t seed) {
    return guard([&] { session_of(s).seed = seed; });
}

nc_status nc_session_query(const nc_session* s, int64_t n_in, int64_t* out_cap) {
    return guard([&] {
        const nc_session& x = session_of(s);
        if (!out_cap) fail(NC_EINVAL, "out_cap must not be null");
        if (n_in < 0 || n_in > ((int64_t)1 << 30)) fail(NC_EINVAL, "n_in must be in 0..2^30");
        if (x.decode && n_in % x.align != 0) fail(NC_EINVAL, "a push of %lld frames is not a multiple of %lld", (long long)n_in, (long long)x.align);
        *out_cap = x.out_elems(x.cap_frames(n_in));
    });
}

nc_status nc_session_pending(const nc_session* s, int64_t* frames) {
    return guard([&] {
        if (!frames) fail(NC_EINVAL, "frames must not be null");
        const nc_session& x = session_of(s);
        *frames = x.P - x.E;
    });
}

nc_status nc_session_push_dev(nc_session* s, const void* in, int64_t n_in, const float* noise, void* out, int64_t out_cap, int64_t* n_out) {
    return guard([&] { step(session_of(s), false, in, n_in, noise, out, out_cap, n_out, false); });
}
nc_status nc_session_push(nc_session* s, const void* in, int64_t n_in, const float* noise, void* out, int64_t out_cap, int64_t* n_out) {
    return guard([&] { host_call(s, [&] { step(*s, true, in, n_in, noise, out, out_cap, n_out, false); }); });
}
nc_status nc_session_flush_dev(nc_session* s, void* out, int64_t out_cap, int64_t* n_out) {
    return guard([&] { step(session_of(s), false, nullptr, 0, nullptr, out, out_cap, n_out, true); });
}
nc_status nc_session_flush(nc_session* s, void* out, int64_t out_cap, int64_t* n_out) {
    return guard([&] { host_call(s, [&] { step(*s, true, nullptr, 0, nullptr, out, out_cap, n_out, true); }); });
}

}  // extern "C"
