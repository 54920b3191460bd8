// Session pool: n_slots independent DAC / SNAC streams on one handle, stepped in one call (include/nc_mi355x.h, "session pool";
// DESIGN.md 4g).
//
// Schedule.  Every slot is one stream of nc_session.hip with B = 1: the same state (SessionState), the same rule (session_check,
// session_move, session_commit of nc_session.h).  A step takes entries (slot, n_in), n_in == 0 being the flush.  The whole call is
// validated and every entry's move is computed from frame counts before anything is launched or any slot changes.  Entries whose move
// runs a window are grouped by the window's width in frames; a group of g entries runs as ONE uniform batch of g rows through the
// existing *_dev launch sequence.  Every conv instance computes a column from the same operands in the same order whichever row of the
// batch it sits in (the premise of the ragged calls, nc_ragged.hip), so a row of a group is the B = 1 window of its slot, bit for bit.
//
// Device work.  Histories live in two pool-owned slabs with a fixed capacity per slot; a slot reads one and writes the other, as a
// session alternates its two buffers.
//   pool_assemble_{i64,f32}  one table-driven launch per step and tensor: a descriptor is a run of the concatenation (history run ++
//                            pushed run ++ zeros) from a start offset to a destination, either a window row or the slot's next history.
//   emit                     the kept columns of a group's output go to the packed output with the table-driven copy of the ragged calls
//                            (RgTables / rg_copy_*: one source run per descriptor is all an emit needs), one launch per group.
// All descriptors of a step are written and bounds-checked on the host first and travel in one pinned image with one asynchronous copy
// (rg_upload).  No LDS, no atomics; profile class NC_KC_ELEM.  The copy is concat_copy (nc_copy.h); the two-half addressing, the slot
// lookup and the grid.y launch loop are nc_pool.h's.
#include <cstring>
#include <map>
#include <vector>

#include "nc_pool.h"
#include "nc_ragged.h"
#include "nc_session.h"

namespace nc {

namespace {

// d[0, n) = (hist[a, a + na) ++ nw[b, b + nb) ++ zeros)[s0, s0 + n), d = (to_hist ? hist : win) + dst.  Elements.
struct PoolSeg { int64_t a, na, b, nb, s0, dst, n, to_hist; };

// blockIdx.y = descriptor, blockIdx.x strides over its run.  `hist` is read and written: no descriptor of a launch writes what another reads
// (a slot's current half is only read, its other half only written).
template <class T>
__device__ __forceinline__ void pool_assemble_body(const PoolSeg* __restrict__ segs, T* hist, const T* nw, T* win) {
    const PoolSeg g = segs[blockIdx.y];
    concat_copy<T>(hist + g.a, g.na, nw + g.b, g.nb, g.s0, (g.to_hist ? hist : win) + g.dst, g.n);
}
__global__ __launch_bounds__(256) void pool_assemble_i64(const PoolSeg* __restrict__ segs, int64_t* hist, const int64_t* nw, int64_t* win) {
    pool_assemble_body<int64_t>(segs, hist, nw, win);
}
__global__ __launch_bounds__(256) void pool_assemble_f32(const PoolSeg* __restrict__ segs, float* hist, const float* nw, float* win) {
    pool_assemble_body<float>(segs, hist, nw, win);
}

// The descriptors of one assembly launch, each checked against the four arrays it addresses before it is accepted.
struct SegTable {
    std::vector<PoolSeg> segs;
    int64_t longest = 0;
    double bytes = 0;
    // hist reads stay in [h_lo, h_hi), hist writes in [x_lo, x_hi) (the slot's two halves), pushed reads in [0, in_n), window writes in [0, win_n)
    void add(const PoolSeg& s, int64_t h_lo, int64_t h_hi, int64_t x_lo, int64_t x_hi, int64_t in_n, int64_t win_n, size_t elt) {
        if (s.n == 0) return;
        const int64_t d_lo = s.to_hist ? x_lo : 0, d_hi = s.to_hist ? x_hi : win_n;
        if (s.n < 0 || s.na < 0 || s.nb < 0 || s.s0 < 0 || (s.na > 0 && (s.a < h_lo || s.a + s.na > h_hi)) || (s.nb > 0 && (s.b < 0 || s.b + s.nb > in_n)) ||
            s.dst < d_lo || s.dst + s.n > d_hi)
            fail(NC_ESTATE, "internal: pool descriptor [%lld + %lld | %lld + %lld] from %lld -> [%lld + %lld] leaves its arrays", (long long)s.a,
                 (long long)s.na, (long long)s.b, (long long)s.nb, (long long)s.s0, (long long)s.dst, (long long)s.n);
        segs.push_back(s);
        longest = std::max(longest, s.n);
        bytes += 2.0 * (double)s.n * (double)elt;
    }
};

template <class T>
void launch_assemble(Codec& m, void (*kernel)(const PoolSeg*, T*, const T*, T*), const SegTable& t, const PoolSeg* dev, T* hist, const T* nw, T* win) {
    if (t.segs.empty()) return;
    const unsigned gx = copy_grid_x(t.longest, sizeof(T));
    ProfScope ps(&m.prof, m.stream, NC_KC_ELEM, 0.0, t.bytes);
    for_grid_y(t.segs.size(), [&](size_t done, size_t cnt) {
        hipLaunchKernelGGL(kernel, dim3(gx, (unsigned)cnt), dim3(256), 0, m.stream, dev + done, hist, nw, win);
        NC_HIP(hipGetLastError());
    });
}

// ---- grouping ----------------------------------------------------------------------------------------------------------------------
struct PoolGroup { int64_t W; std::vector<int> entries; };

// Entries with width[i] > 0 by width, narrowest first, in entry order inside a width; a width with more than max_rows entries is split.
std::vector<PoolGroup> group_windows(int n, const int64_t* width, int max_rows, int32_t* group_of) {
    std::map<int64_t, std::vector<int>> by_width;
    for (int i = 0; i < n; ++i) {
        if (group_of) group_of[i] = -1;
        if (width[i] > 0) by_width[width[i]].push_back(i);
    }
    std::vector<PoolGroup> groups;
    for (const auto& w : by_width)
        for (size_t r = 0; r < w.second.size(); r += (size_t)max_rows) {
            PoolGroup g{w.first, {}};
            g.entries.assign(w.second.begin() + (std::ptrdiff_t)r, w.second.begin() + (std::ptrdiff_t)std::min(w.second.size(), r + (size_t)max_rows));
            if (group_of)
                for (int e : g.entries) group_of[e] = (int32_t)groups.size();
            groups.push_back(std::move(g));
        }
    return groups;
}

}  // namespace

}  // namespace nc

using namespace nc;

// the opaque pool of the C ABI
struct nc_session_pool {
    SessionGeom g;                // one stream of the pool (B = 1)
    struct Slot {
        SessionState st;
        uint64_t seed = 0;
    };
    std::vector<Slot> slots;
    TwoHalves main, noise;        // of hist and nhist: a slot's history is in half st.cur, its next one goes to the other half
    DevBuf hist, nhist;           // [2][n_slots][cap]
    DevBuf in_stage, nz_stage, out_stage;   // host-pointer calls and drawn noise

    int64_t n_slots() const { return (int64_t)slots.size(); }
    static constexpr const char* kNull = "null session pool";
    static constexpr const char* kRange = "slot %d is outside 0..%lld";
    static constexpr int kRangeLast = 1;
};

namespace {

struct Entry {
    int slot = 0;
    bool flush = false;
    SessionMove mv{};
    int group = -1, row = 0;
    int64_t in_off = 0, nz_off = 0, out_off = 0;
};

// Every entry checked against its slot and moved on frame counts alone; nothing changes.
std::vector<Entry> plan_entries(nc_session_pool& p, int32_t n, const int32_t* slots, const int64_t* n_in) {
    if (n <= 0 || !slots || !n_in) fail(NC_EINVAL, "n must be positive, slots and n_in must not be null");
    if (n > p.n_slots()) fail(NC_EINVAL, "%d entries for %lld slots: a slot appears at most once per step", n, (long long)p.n_slots());
    std::vector<char> seen((size_t)p.n_slots(), 0);
    std::vector<Entry> es((size_t)n);
    for (int i = 0; i < n; ++i) {
        Entry& e = es[(size_t)i];
        const nc_session_pool::Slot& s = slot_of(p, slots[i]);
        if (seen[(size_t)slots[i]]) fail(NC_EINVAL, "slot %d appears twice in one step", slots[i]);
        seen[(size_t)slots[i]] = 1;
        if (n_in[i] < 0) fail(NC_EINVAL, "entry %d: n_in must not be negative (0: flush)", i);
        e.slot = slots[i];
        e.flush = n_in[i] == 0;
        session_check(p.g, s.st, n_in[i], e.flush);
        e.mv = session_move(p.g, s.st, n_in[i], e.flush);
    }
    return es;
}

void pool_step(nc_session_pool& p, bool host, int32_t n, const int32_t* slots, const int64_t* n_in, const void* in, const float* noise, void* out,
               int64_t out_cap, int64_t* n_out) {
    const SessionGeom& g = p.g;
    Codec& m = codec_of(g.h);
    if (!out || !n_out) fail(NC_EINVAL, "out_packed and n_out must not be null");
    std::vector<Entry> es = plan_entries(p, n, slots, n_in);
    const int rps = g.rows(), ors = g.out_rows();   // rows of a slot in the pushed tensor / in the output
    int64_t in_n = 0, nz_n = 0, out_n = 0;
    for (Entry& e : es) {
        e.in_off = in_n; e.nz_off = nz_n; e.out_off = out_n;
        in_n += (int64_t)rps * g.main.total(e.mv.new_u);
        if (g.with_noise) nz_n += g.noise.total(e.mv.new_u);
        out_n += (int64_t)ors * e.mv.nout;
    }
    if (in_n > 0 && !in) fail(NC_EINVAL, "in_packed must not be null");
    if (!m.loaded) fail(NC_ESTATE, "weights not loaded (call nc_codec_load_weights first)");
    if (out_cap < out_n) fail(NC_EINVAL, "out_cap %lld is below what nc_session_pool_query asks for (%lld)", (long long)out_cap, (long long)out_n);

    // ---- groups and where their windows lie (each group's rows start on a 256-byte boundary)
    std::vector<int64_t> width((size_t)n);
    for (int i = 0; i < n; ++i) width[(size_t)i] = es[(size_t)i].mv.run ? es[(size_t)i].mv.Wf : 0;
    const int max_rows = m.ragged_max_windows > 0 ? m.ragged_max_windows : kRaggedDefaultMaxWindows;
    const std::vector<PoolGroup> groups = group_windows(n, width.data(), max_rows, nullptr);
    const int64_t per = g.decode ? 1 : g.hop;
    std::vector<int64_t> wbase(groups.size()), nbase(groups.size());
    int64_t win_n = 0, nwin_n = 0, lat_n = 0, res_n = 0;   // window tensors of all groups; latents and result of the largest group
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        const int64_t cnt = (int64_t)groups[gi].entries.size(), Wf = groups[gi].W;
        for (size_t r = 0; r < groups[gi].entries.size(); ++r) { es[(size_t)groups[gi].entries[r]].group = (int)gi; es[(size_t)groups[gi].entries[r]].row = (int)r; }
        wbase[gi] = win_n; nbase[gi] = nwin_n;
        win_n = round_up(win_n + cnt * rps * g.main.total(Wf * per), kAlign);
        if (g.with_noise) nwin_n = round_up(nwin_n + cnt * g.noise.total(Wf), kAlign);
        const SessionMove& mv = es[(size_t)groups[gi].entries[0]].mv;
        if (g.decode) {
            res_n = std::max(res_n, cnt * mv.Lw);
            if (g.dac) lat_n = std::max(lat_n, cnt * (int64_t)static_cast<DacModel&>(m).latent * Wf);
        } else {
            res_n = std::max(res_n, cnt * ors * g.codes.total(Wf));
        }
    }

    // ---- every descriptor of the step
    SegTable tm, tz;
    RgTables te;
    const size_t elt = g.elt();
    for (const Entry& e : es) {
        const SessionMove& mv = e.mv;
        const int cur = p.slots[(size_t)e.slot].st.cur;
        const int64_t h_lo = p.main.at(cur, e.slot), x_lo = p.main.at(1 - cur, e.slot);
        const Lay lh = lay_of(g.main, mv.hist_u, rps, false), ln = lay_of(g.main, mv.new_u, rps, g.main.row_major), lx = lay_of(g.main, mv.next_u, rps, false);
        Lay lw{};
        int64_t grows = 0;
        if (mv.run) {
            grows = (int64_t)groups[(size_t)e.group].entries.size() * rps;
            lw = lay_of(g.main, mv.win_u, grows, g.main.row_major);
        }
        for (int i = 0; i < g.main.nl; ++i)
            for (int q = 0; q < rps; ++q) {
                const int64_t a = h_lo + lh.base[i] + q * lh.len[i], b = e.in_off + ln.base[i] + q * ln.pitch[i];
                if (mv.run)
                    tm.add({a, lh.len[i], b, ln.len[i], 0, wbase[(size_t)e.group] + lw.base[i] + ((int64_t)e.row * rps + q) * lw.pitch[i], lw.len[i], 0}, h_lo,
                           h_lo + p.main.cap, x_lo, x_lo + p.main.cap, in_n, win_n, elt);
                tm.add({a, lh.len[i], b, ln.len[i], lh.len[i] + ln.len[i] - lx.len[i], x_lo + lx.base[i] + q * lx.len[i], lx.len[i], 1}, h_lo, h_lo + p.main.cap,
                       x_lo, x_lo + p.main.cap, in_n, win_n, elt);
            }
        if (g.with_noise) {
            const int64_t zh = p.noise.at(cur, e.slot), zx = p.noise.at(1 - cur, e.slot);
            const Lay zl = lay_of(g.noise, mv.hist_u, 1, false), zn = lay_of(g.noise, mv.new_u, 1, false), zz = lay_of(g.noise, mv.next_u, 1, false);
            Lay zw{};
            if (mv.run) zw = lay_of(g.noise, mv.Wf, (int64_t)groups[(size_t)e.group].entries.size(), false);
            for (int i = 0; i < g.noise.nl; ++i) {
                const int64_t a = zh + zl.base[i], b = e.nz_off + zn.base[i];
                if (mv.run)
                    tz.add({a, zl.len[i], b, zn.len[i], 0, nbase[(size_t)e.group] + zw.base[i] + (int64_t)e.row * zw.pitch[i], zw.len[i], 0}, zh, zh + p.noise.cap, zx,
                           zx + p.noise.cap, nz_n, nwin_n, 4);
                tz.add({a, zl.len[i], b, zn.len[i], zl.len[i] + zn.len[i] - zz.len[i], zx + zz.base[i], zz.len[i], 1}, zh, zh + p.noise.cap, zx, zx + p.noise.cap, nz_n,
                       nwin_n, 4);
            }
        }
    }
    for (const PoolGroup& gr : groups) {   // one emit launch per group: kept columns -> the entry's place in the packed output
        const int64_t cnt = (int64_t)gr.entries.size(), Wf = gr.W;
        const SessionMove& m0 = es[(size_t)gr.entries[0]].mv;
        const int64_t row_n = g.decode ? m0.Lw : g.codes.total(Wf);
        te.begin(cnt * ors * row_n, out_n);
        for (int ei : gr.entries) {
            const Entry& e = es[(size_t)ei];
            const SessionMove& mv = e.mv;
            if (g.decode) {
                te.add((int64_t)e.row * row_n + mv.k_off * g.H, e.out_off, mv.nout);
            } else {
                const Lay lw = lay_of(g.codes, Wf, cnt * ors, g.codes.row_major), lk = lay_of(g.codes, mv.ke, ors, true);
                for (int i = 0; i < g.codes.nl; ++i)
                    for (int q = 0; q < ors; ++q)
                        te.add(lw.base[i] + ((int64_t)e.row * ors + q) * lw.pitch[i] + g.codes.len(i, mv.k_off), e.out_off + lk.base[i] + q * mv.nout, lk.len[i]);
            }
        }
        te.end();
    }
    const size_t tm_bytes = tm.segs.size() * sizeof(PoolSeg), tz_bytes = tz.segs.size() * sizeof(PoolSeg);
    te.extra.resize(tm_bytes + tz_bytes);
    if (tm_bytes) std::memcpy(te.extra.data(), tm.segs.data(), tm_bytes);
    if (tz_bytes) std::memcpy(te.extra.data() + tm_bytes, tz.segs.data(), tz_bytes);

    // ---- launches
    m.use_device();
    const void* src = in;
    if (host && in_n > 0) {
        p.in_stage.reserve((size_t)in_n * elt);
        NC_HIP(hipMemcpyAsync(p.in_stage.p, in, (size_t)in_n * elt, hipMemcpyHostToDevice, m.stream));
        src = p.in_stage.p;
    }
    const float* nz = noise;
    if (g.with_noise && nz_n > 0) {
        if (!noise) {   // every pushing entry draws its block from (slot seed, frame position), as a single session does
            p.nz_stage.reserve((size_t)nz_n * 4);
            for (const Entry& e : es)
                if (e.mv.new_u > 0) launch_randn(p.nz_stage.as<float>() + e.nz_off, g.noise.total(e.mv.new_u), mix_seed(p.slots[(size_t)e.slot].seed, p.slots[(size_t)e.slot].st.P), m.stream);
            nz = p.nz_stage.as<float>();
        } else if (host) {
            p.nz_stage.reserve((size_t)nz_n * 4);
            NC_HIP(hipMemcpyAsync(p.nz_stage.p, noise, (size_t)nz_n * 4, hipMemcpyHostToDevice, m.stream));
            nz = p.nz_stage.as<float>();
        }
    }
    DevBuf& wbuf = g.decode ? m.ck_codes : m.ck_in;     // the windows of all groups
    DevBuf& rbuf = g.decode ? m.ck_out : m.ck_codes;    // one group's result, reused by the next group
    wbuf.reserve(std::max<size_t>(16, (size_t)win_n * elt));
    rbuf.reserve(std::max<size_t>(16, (size_t)res_n * (g.decode ? 4 : 8)));
    if (g.with_noise) m.ck_noise.reserve(std::max<size_t>(16, (size_t)nwin_n * 4));
    if (lat_n > 0) m.ck_a.reserve((size_t)lat_n * 4);
    void* dst = out;
    if (host) {
        p.out_stage.reserve(std::max<size_t>(16, (size_t)out_n * (g.decode ? 4 : 8)));
        dst = p.out_stage.p;
    }
    const char* ex = rg_upload(m, te);
    const PoolSeg* dm = reinterpret_cast<const PoolSeg*>(ex);
    const PoolSeg* dz = reinterpret_cast<const PoolSeg*>(ex + tm_bytes);
    if (g.decode) launch_assemble<int64_t>(m, pool_assemble_i64, tm, dm, p.hist.as<int64_t>(), static_cast<const int64_t*>(src), wbuf.as<int64_t>());
    else launch_assemble<float>(m, pool_assemble_f32, tm, dm, p.hist.as<float>(), static_cast<const float*>(src), wbuf.as<float>());
    if (g.with_noise) launch_assemble<float>(m, pool_assemble_f32, tz, dz, p.nhist.as<float>(), nz, m.ck_noise.as<float>());
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        const int cnt = (int)groups[gi].entries.size();
        const int64_t Wf = groups[gi].W;
        if (g.decode) {
            const int64_t* win = wbuf.as<int64_t>() + wbase[gi];
            if (g.dac) {
                DacModel& d = static_cast<DacModel&>(m);
                d.from_codes_dev(win, cnt, g.nq, Wf, m.ck_a.as<float>());
                d.decode_dev(m.ck_a.as<float>(), cnt, Wf, rbuf.as<float>());
            } else {
                static_cast<SnacModel&>(m).decode_dev(win, cnt, Wf, g.with_noise ? m.ck_noise.as<float>() + nbase[gi] : nullptr, 0, rbuf.as<float>());
            }
            rg_copy_f32(m, te, gi, rbuf.as<float>(), static_cast<float*>(dst));
        } else {
            const float* win = wbuf.as<float>() + wbase[gi];
            if (g.dac) static_cast<DacModel&>(m).encode_dev(win, cnt, Wf * g.hop, 0, 0, rbuf.as<int64_t>(), nullptr, nullptr);
            else static_cast<SnacModel&>(m).encode_dev(win, cnt, Wf * g.hop, rbuf.as<int64_t>(), nullptr, nullptr, true);
            rg_copy_i64(m, te, gi, rbuf.as<int64_t>(), static_cast<int64_t*>(dst));
        }
    }
    if (host && out_n > 0) NC_HIP(hipMemcpyAsync(out, dst, (size_t)out_n * (g.decode ? 4 : 8), hipMemcpyDeviceToHost, m.stream));
    // ---- the slots move on only once everything is queued
    for (int i = 0; i < n; ++i) {
        session_commit(p.slots[(size_t)es[(size_t)i].slot].st, es[(size_t)i].mv, es[(size_t)i].flush);
        n_out[i] = es[(size_t)i].mv.nout;
    }
}

}  // namespace

// ================================================================================================ C ABI
extern "C" {

nc_status nc_session_pool_plan(const nc_halo* halo, int32_t decode, int32_t n, const int64_t* pushed, const int64_t* emitted, const int64_t* push_frames,
                               int32_t max_rows, nc_session_step* steps, int32_t* group_of, int32_t* n_groups) {
    return guard([&] {
        if (!halo || !pushed || !emitted || !push_frames || !steps || !group_of || !n_groups) fail(NC_EINVAL, "null pointer");
        if (n <= 0 || max_rows < 0) fail(NC_EINVAL, "n must be positive and max_rows must not be negative (0 = default)");
        int64_t hl, hr;
        session_halos(*halo, decode != 0, hl, hr);
        const int64_t al = halo->align;
        std::vector<int64_t> width((size_t)n);
        for (int i = 0; i < n; ++i) {
            const int64_t P = pushed[i], E = emitted[i], f = push_frames[i];
            if (P < 0 || E < 0 || E > P || P % al != 0 || E % al != 0 || P > ((int64_t)1 << 40))
                fail(NC_EINVAL, "stream %d: pushed %lld / emitted %lld is no state of a stream aligned to %lld", i, (long long)P, (long long)E, (long long)al);
            if (f < 0 || f % al != 0 || f > ((int64_t)1 << 40)) fail(NC_EINVAL, "stream %d: a push of %lld frames is not a multiple of %lld", i, (long long)f, (long long)al);
            if (f == 0 && P == 0) fail(NC_EINVAL, "stream %d: nothing to flush", i);
            const SsStep st = f == 0 ? step_flush(hl, E, P) : step_push(hl, hr, al, E, P + f);
            steps[i] = {st.w0, st.w1, st.k0, st.k1, P + f - st.h0n};
            width[(size_t)i] = st.k1 > st.k0 ? st.w1 - st.w0 : 0;
        }
        *n_groups = (int32_t)group_windows(n, width.data(), max_rows > 0 ? max_rows : kRaggedDefaultMaxWindows, group_of).size();
    });
}

nc_status nc_session_pool_create(nc_codec* h, int32_t decode, int32_t n_slots, int32_t n_q, nc_session_pool** out) {
    return guard([&] {
        if (!out) fail(NC_EINVAL, "out must not be null");
        *out = nullptr;
        std::unique_ptr<nc_session_pool> p(new nc_session_pool);
        session_geom(h, decode != 0, 1, n_q, p->g);
        if (n_slots <= 0 || n_slots > 65536) fail(NC_EINVAL, "n_slots must be in 1..65536");
        p->slots.resize((size_t)n_slots);
        // a stream holds at most hl + hr + align frames (invariant 1); encode: as samples, plus less than one hop * align buffered
        const SessionGeom& g = p->g;
        const int64_t cap_f = g.hl + g.hr + g.align;
        p->main = {n_slots, round_up((int64_t)g.rows() * g.main.total(g.decode ? cap_f : cap_f * g.hop + g.unit()), 4)};
        if (g.with_noise) p->noise = {n_slots, round_up(g.noise.total(cap_f), 4)};
        Codec& m = codec_of(h);
        m.use_device();
        p->hist.reserve((size_t)p->main.elems() * g.elt());
        if (g.with_noise) p->nhist.reserve((size_t)p->noise.elems() * 4);
        *out = p.release();
    });
}

nc_status nc_session_pool_destroy(nc_session_pool* p) {
    return guard([&] { delete p; });
}

nc_status nc_session_pool_reset_slot(nc_session_pool* p, int32_t slot) {
    return guard([&] { reset_keep_cur(slot_of(pool_of(p), slot).st); });
}

nc_status nc_session_pool_set_seed(nc_session_pool* p, int32_t slot, uint64_t seed) {
    return guard([&] { slot_of(pool_of(p), slot).seed = seed; });
}

nc_status nc_session_pool_pending(const nc_session_pool* p, int32_t slot, int64_t* frames) {
    return guard([&] {
        if (!frames) fail(NC_EINVAL, "frames must not be null");
        const SessionState& s = slot_of(pool_of(p), slot).st;
        *frames = s.P - s.E;
    });
}

nc_status nc_session_pool_query(const nc_session_pool* p, int32_t n, const int32_t* slots, const int64_t* n_in, int64_t* n_out) {
    return guard([&] {
        if (!n_out) fail(NC_EINVAL, "n_out must not be null");
        const std::vector<Entry> es = plan_entries(pool_of(p), n, slots, n_in);
        for (int i = 0; i < n; ++i) n_out[i] = es[(size_t)i].mv.nout;
    });
}

nc_status nc_session_pool_step_dev(nc_session_pool* p, int32_t n, const int32_t* slots, const int64_t* n_in, const void* in_packed,
                                   const float* noise_packed, void* out_packed, int64_t out_cap, int64_t* n_out) {
    return guard([&] { pool_step(pool_of(p), false, n, slots, n_in, in_packed, noise_packed, out_packed, out_cap, n_out); });
}

nc_status nc_session_pool_step(nc_session_pool* p, int32_t n, const int32_t* slots, const int64_t* n_in, const void* in_packed,
                               const float* noise_packed, void* out_packed, int64_t out_cap, int64_t* n_out) {
    return guard([&] {
        nc_session_pool& x = pool_of(p);
        Codec& m = codec_of(x.g.h);
        OwnStreamScope own(m);
        pool_step(x, true, n, slots, n_in, in_packed, noise_packed, out_packed, out_cap, n_out);
        NC_HIP(hipStreamSynchronize(m.stream));
    });
}

// test hook: concat_copy (nc_copy.h) alone, as ONE pool_assemble launch over n_desc descriptors (a_off, na, b_off, nb, s0, dst_off, n)
nc_status nc_op_concat_copy(int device_index, int32_t elt, const void* a, int64_t a_n, const void* b, int64_t b_n, void* dst, int64_t dst_n,
                            const int64_t* desc, int64_t n_desc) {
    return guard([&] {
        if (!a || !b || !dst || !desc) fail(NC_EINVAL, "null argument");
        if ((elt != 4 && elt != 8) || a_n <= 0 || b_n <= 0 || dst_n <= 0 || n_desc <= 0 || n_desc > 65535)
            fail(NC_EINVAL, "elt must be 4 or 8, the arrays non-empty, n_desc in 1..65535 (one launch)");
        use_checked_device(device_index);
        SegTable t;
        for (int64_t i = 0; i < n_desc; ++i) {
            const int64_t* d = desc + 7 * i;
            t.add({d[0], d[1], d[2], d[3], d[4], d[5], d[6], 0}, 0, a_n, 0, 0, b_n, dst_n, (size_t)elt);
        }
        if (t.segs.empty()) return;
        DevBuf da, db, dd, ds;
        h2d(da, a, (size_t)a_n * elt, nullptr);
        h2d(db, b, (size_t)b_n * elt, nullptr);
        h2d(dd, dst, (size_t)dst_n * elt, nullptr);
        h2d(ds, t.segs.data(), t.segs.size() * sizeof(PoolSeg), nullptr);
        const dim3 grid(copy_grid_x(t.longest, (size_t)elt), (unsigned)t.segs.size());
        if (elt == 4) hipLaunchKernelGGL(pool_assemble_f32, grid, dim3(256), 0, nullptr, ds.as<PoolSeg>(), da.as<float>(), db.as<float>(), dd.as<float>());
        else hipLaunchKernelGGL(pool_assemble_i64, grid, dim3(256), 0, nullptr, ds.as<PoolSeg>(), da.as<int64_t>(), db.as<int64_t>(), dd.as<int64_t>());
        NC_HIP(hipGetLastError());
        NC_HIP(hipMemcpy(dst, dd.p, (size_t)dst_n * elt, hipMemcpyDeviceToHost));
    });
}

}  // extern "C"
