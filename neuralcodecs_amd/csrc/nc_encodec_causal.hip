// Encodec causal streams: Encode / Decode of live streams on a CAUSAL model without segmentation (the 24 kHz preset), the SLSTM's (h, c)
// carried from call to call (include/nc_mi355x.h, "Encodec causal streams").  Reference: Encodec.Encode / Encodec.Decode
// (Models/Encodec.cs:259-285, 213-235), SLSTM.forward (Modules/Encodec/SLSTM.cs:40-57).
// Why it is exact.  With causal = 1 every SConv1d pads on the left only (plus the extra right pad of the clip's true end), every
// SConvTranspose1d trims on the right only, and the SLSTM runs forward: output t of any layer is a function of inputs <= t.  A window of
// the stream that starts on a hop multiple is phase-aligned with the one-clip call in every strided layer, so its outputs differ from the
// one-clip call's only where their receptive field reaches the window's left edge (or its own left reflect pad) -- the first halo frames,
// which are dropped.  The LSTM is a recurrence: steps [a, b) from the state behind step a - 1 are the steps [a, b) of the whole run,
// launch for launch (lstm_layer_steps, the step-wise form, whose arithmetic is the persistent form's bit for bit).  The last encoder
// convolution and the first decoder convolution are causal k = 7 convolutions: they run on the carried K - 1 inputs + the new ones.
// Every kernel computes an output element by one fixed sequence of operations whatever the batch, the row length or the position in a
// tile (the batch invariance the ragged and session paths rest on), so equal inputs give equal bits.
// State per slot (device): the input not yet consumed + the left context (PCM from halo_e frames before the next frame | the last code
// frames), double-buffered in two halves so that no launch reads what it writes; (h, c) of every LSTM layer; the last LSTM-output frames
// (K - 1 for the encoder's last convolution | halo_d for the decoder's up-stack).
// Kernels (new): cz_copy2d_kernel -- table-driven 2-D block copies (window gather, carry rewrite, concatenation of carried and new
// frames, carry update); cz_state_gather_kernel / cz_state_scatter_kernel -- the LSTM state rows of a batch by slot index to and from
// the unit-major [C][N] layout of lstm_step_kernel.  No LDS, no atomics, no workgroup waits for another; vector stores only.  All tables
// of a step are written and bounds-checked on the host before anything is launched and travel in one pinned image (nc_ragged.h).  The
// pool's host scaffold (two-half carry, slot lookup, a step's state refusals, host-pointer staging) is nc_pool.h, shared with the stream pool.
#include <algorithm>
#include <cstring>
#include <tuple>

#include "nc_encodec_rows.h"
#include "nc_guard.h"
#include "nc_pool.h"
#include "nc_ragged.h"

using namespace nc;

namespace {

// ---- kernels -----------------------------------------------------------------------------------------------------------------------
// One 2-D block: dst[dst + r * dst_rs + c] = src[src + r * src_rs + c] for r < rows, c < cols.  Elements.
struct CzJob { int64_t src, dst, src_rs, dst_rs, rows, cols; };

// blockIdx.y = job, blockIdx.x strides over its elements.  src and dst never overlap within a launch (a slot's carry is read from one
// half and written to the other; every other pair is two different buffers).
template <class T>
__global__ __launch_bounds__(256) void cz_copy2d_kernel(const CzJob* __restrict__ jobs, const T* __restrict__ src, T* __restrict__ dst) {
    const CzJob j = jobs[blockIdx.y];
    const int64_t total = j.rows * j.cols, nthr = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += nthr) {
        const int64_t r = i / j.cols, c = i - r * j.cols;
        dst[j.dst + r * j.dst_rs + c] = src[j.src + r * j.src_rs + c];
    }
}

// LSTM state of one layer for the N rows of a batch.  idx[2 b] = the row's slot, idx[2 b + 1] != 0: a new stream (zero state).
// Slot layout [slot][layer][C]; batch layout [C][N], unit-major (lstm_step_kernel's).
__global__ __launch_bounds__(256) void cz_state_gather_kernel(const int32_t* __restrict__ idx, const float* __restrict__ hs, const float* __restrict__ cs,
                                                              float* __restrict__ h0, float* __restrict__ c0, int N, int C, int nl, int li) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)C * N) return;
    const int b = (int)(i % N), j = (int)(i / N);
    const int64_t s = ((int64_t)idx[2 * b] * nl + li) * C + j;
    const bool fresh = idx[2 * b + 1] != 0;
    h0[i] = fresh ? 0.0f : hs[s];
    c0[i] = fresh ? 0.0f : cs[s];
}
__global__ __launch_bounds__(256) void cz_state_scatter_kernel(const int32_t* __restrict__ idx, const float* __restrict__ hT, const float* __restrict__ cT,
                                                               float* __restrict__ hs, float* __restrict__ cs, int N, int C, int nl, int li) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)C * N) return;
    const int b = (int)(i % N), j = (int)(i / N);
    const int64_t s = ((int64_t)idx[2 * b] * nl + li) * C + j;
    hs[s] = hT[i];
    cs[s] = cT[i];
}

// SLSTM.forward on x [N,C,T] from carried state: per layer, the rows' (h, c) gathered from the slots, T fresh launches of the step-wise
// form (lstm_layer_steps), the state behind the last step scattered back.  d_idx: [N][2] on the device; hs / cs: [slots][layers][C].
float* lstm_run_carried(EncodecModel& m, Lstm& l, const float* x, int N, int64_t T, bool elu_out, const int32_t* d_idx, float* hs, float* cs) {
    const int C = l.C, nl = (int)l.layers.size();
    if (FILE* lf = launch_log()) {
        std::fprintf(lf, "lstm carried C=%d layers=%d T=%lld\n", C, nl, (long long)T);
        std::fflush(lf);
    }
    const unsigned grid = (unsigned)(((int64_t)C * N + 255) / 256);
    const float* in = x;
    float* out = const_cast<float*>(x);
    for (int li = 0; li < nl; ++li) {
        const bool last = li + 1 == nl;
        out = m.alloc((size_t)N * C * T);
        float* h0 = m.alloc((size_t)C * N);
        float* h1 = m.alloc((size_t)C * N);
        float* c0 = m.alloc((size_t)C * N);
        hipLaunchKernelGGL(cz_state_gather_kernel, dim3(grid), dim3(256), 0, m.stream, d_idx, hs, cs, h0, c0, N, C, nl, li);
        NC_HIP(hipGetLastError());
        const float* hT = lstm_layer_steps(m, *l.layers[li], C, in, last ? x : nullptr, out, h0, h1, c0, N, T, last && elu_out);
        hipLaunchKernelGGL(cz_state_scatter_kernel, dim3(grid), dim3(256), 0, m.stream, d_idx, hT, c0, hs, cs, N, C, nl, li);
        NC_HIP(hipGetLastError());
        in = out;
    }
    return out;
}

// ---- geometry ----------------------------------------------------------------------------------------------------------------------
struct CzGeom {
    int64_t hop = 1, halo_e = 0, halo_d = 0, min_e = 1, min_d = 1, carry_e = 0, kin_d = 0, carry_d = 0, taint_e = 0, taint_d = 0;
};

// the encoder's convolutional front on L samples by the pad plans alone: frames at the LSTM input; *d9: some layer took SConv1d's small-input path
int64_t front_frames(const EncodecModel& m, int64_t L, bool* d9) {
    auto step = [&](int k, int s) {
        const EncodecModel::Plan p = m.plan_sconv(L, k, s, 1);
        if (p.Lz != L) *d9 = true;
        L = p.Lout;
    };
    step(m.cfg.kernel_size, 1);
    for (int i = m.cfg.n_ratios - 1; i >= 0; --i) {
        step(m.cfg.residual_kernel_size, 1);
        step(2 * m.cfg.ratios[i], m.cfg.ratios[i]);
    }
    return L;
}
// a stride-1 causal convolution of k taps on F frames (the encoder's last, the decoder's first)
bool conv_d9(const EncodecModel& m, int64_t F, int k) { return m.plan_sconv(F, k, 1, 1).Lz != F; }
// the decoder behind its LSTM on F frames: decoded samples
int64_t tail_samples(const EncodecModel& m, int64_t F, bool* d9) {
    int64_t L = F;
    auto step = [&](int k) {
        const EncodecModel::Plan p = m.plan_sconv(L, k, 1, 1);
        if (p.Lz != L) *d9 = true;
        L = p.Lout;
    };
    for (int i = 0; i < m.cfg.n_ratios; ++i) {
        L = L * m.cfg.ratios[i];   // (L - 1) r + 2 r, trimmed by r on the right (trimRightRatio = 1)
        step(m.cfg.residual_kernel_size);
    }
    step(m.cfg.last_kernel_size);
    return L;
}

// Admission and the closed forms.  t = leading outputs of a layer that the window's left edge (or the window's own left
// reflect pad) can reach, given t such inputs: a causal convolution of k taps and stride s pads k - s on the left, output j reads inputs
// j s - (k - s) .. j s + s - 1, so it is reached iff j s < t + k - s; a transposed convolution of K taps and stride s sums inputs
// ceil((p - K + 1) / s) .. floor(p / s) into output p, which is reached iff p < (t - 1) s + K.
CzGeom geom_of(const EncodecModel& m, const char* what) {
    const nc_encodec_config& c = m.cfg;
    if (!c.causal) fail(NC_EUNSUPPORTED, "%s: the model is not causal (causal == 0): its convolutions look to the right, so a stream's past is not final", what);
    if (c.segment_length != 0)
        fail(NC_EUNSUPPORTED, "%s: the model is segmented (segment_length != 0): its streams run segment by segment through nc_encodec_stream_pool_*", what);
    if (c.normalize) fail(NC_EUNSUPPORTED, "%s: the model normalises (normalize != 0): the RMS scale of a clip needs the whole clip", what);
    if (c.time_group_norm) fail(NC_EUNSUPPORTED, "%s: the model's norm is time_group_norm: its statistics need the whole clip", what);
    CzGeom g;
    g.hop = m.hop;
    auto conv = [](int64_t t, int k, int s) { return (k - s > 0 || t > 0) ? (t + (k - s) + s - 1) / s : t; };
    int64_t t = conv(0, c.kernel_size, 1);
    for (int i = c.n_ratios - 1; i >= 0; --i) {
        t = conv(t, c.residual_kernel_size, 1);
        t = conv(t, 2 * c.ratios[i], c.ratios[i]);
    }
    g.taint_e = t;
    t = 0;
    for (int i = 0; i < c.n_ratios; ++i) {
        t = (t - 1) * c.ratios[i] + 2 * c.ratios[i];
        t = conv(t, c.residual_kernel_size, 1);
    }
    g.taint_d = conv(t, c.last_kernel_size, 1);
    g.halo_e = g.taint_e;
    g.halo_d = (g.taint_d + g.hop - 1) / g.hop;
    g.carry_e = c.last_kernel_size - 1;
    g.kin_d = c.kernel_size - 1;
    // minimum window: no layer of a window that is run may take the small-input path, which the whole stream would not take
    auto enc_ok = [&](int64_t L) { bool d9 = false; front_frames(m, L, &d9); return !d9; };
    auto dec_ok = [&](int64_t F) { bool d9 = false; tail_samples(m, F, &d9); return !d9; };
    for (int guard_i = 0; guard_i < 64 && !(enc_ok(g.halo_e * g.hop + 1) && enc_ok((g.halo_e + 1) * g.hop)); ++guard_i) ++g.halo_e;
    for (int guard_i = 0; guard_i < 64 && !dec_ok(g.halo_d + 1); ++guard_i) ++g.halo_d;
    g.min_e = 1;
    while (g.min_e < 4096 && !(enc_ok(g.min_e * g.hop) && !conv_d9(m, g.min_e, c.last_kernel_size))) ++g.min_e;
    g.min_e = std::max({g.min_e, g.halo_e, g.carry_e});
    g.min_d = 1;
    while (g.min_d < 4096 && !(dec_ok(g.min_d) && !conv_d9(m, g.min_d, c.kernel_size))) ++g.min_d;
    g.min_d = std::max({g.min_d, g.halo_d, g.kin_d});
    g.carry_d = std::max(g.kin_d, g.min_d - 1);
    if (!enc_ok((g.halo_e + 1) * g.hop) || !dec_ok(g.halo_d + 1) || g.min_e >= 4096 || g.min_d >= 4096 || conv_d9(m, g.carry_e + 1, c.last_kernel_size) ||
        conv_d9(m, g.kin_d + 1, c.kernel_size))
        fail(NC_EUNSUPPORTED, "%s: no window of this layout avoids SConv1d's small-input path", what);
    return g;
}

// ---- planner -----------------------------------------------------------------------------------------------------------------------
struct CzEntry {
    int32_t id = 0;                         // the slot (pool) or the stream's index (planner)
    int64_t T0 = 0, E0 = 0, n_in = 0;       // before the step: samples | frames received, frames emitted | decoded
    bool flush = false;
    int64_t T1 = 0, E1 = 0;                 // after it
    int64_t n_new = 0, n_out = 0;           // frames the entry's row runs; code frames | samples per channel it emits
    int64_t in_off = 0, out_off = 0;        // prefix sums over the entries: samples | frames in (per channel | codebook), frames | samples out
    int row = -1;                           // its row in P.rows (launch order), -1: the entry only appends
};
struct CzRow {
    int32_t entry = 0;
    bool one_clip = false, first = false;
    int64_t start = 0, width = 0, n_new = 0;
    int batch = 0, row = 0;
    auto key() const { return std::make_tuple(width, n_new, (int)first, (int)one_clip); }
};
struct CzBatch { size_t first = 0, count = 0; };
struct CzPlan {
    std::vector<CzEntry> e;
    std::vector<CzRow> rows;
    std::vector<CzBatch> batches;
    int64_t total_in = 0, total_out = 0;
};

CzPlan make_plan(const EncodecModel& m, const CzGeom& g, bool decode, int n, const int32_t* ids, const int64_t* T0, const int64_t* E0, const int64_t* n_in,
                 const int32_t* flush, int32_t max_rows, const char* what) {
    const int64_t cap_rows = er_max_rows(max_rows, what);
    CzPlan P;
    P.e.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        CzEntry& e = P.e[(size_t)i];
        e.id = ids ? ids[i] : i;
        e.T0 = T0[i]; e.E0 = E0[i]; e.n_in = n_in[i]; e.flush = flush && flush[i] != 0;
        if (e.n_in < 0) fail(NC_EINVAL, "%s: slot %d: n_in is negative", what, e.id);
        if (e.n_in > ((int64_t)1 << 28) || e.T0 > ((int64_t)1 << 40)) fail(NC_EINVAL, "%s: slot %d: stream too long", what, e.id);
        e.T1 = e.T0 + e.n_in;
        if (e.flush && e.T1 == 0) fail(NC_EINVAL, "%s: slot %d: a flush of a stream that has received nothing", what, e.id);
        e.in_off = P.total_in; e.out_off = P.total_out;
        P.total_in += e.n_in;
        CzRow r;
        r.entry = i;
        bool runs = false;
        if (!decode) {
            const int64_t F1 = e.T1 / g.hop;
            if (e.E0 == 0) {
                if (F1 >= g.min_e) { runs = true; r.first = true; r.start = 0; r.width = e.flush ? e.T1 : F1 * g.hop; r.n_new = e.flush ? m.frames_for(e.T1) : F1; }
                else if (e.flush) { runs = true; r.one_clip = true; r.start = 0; r.width = e.T1; r.n_new = m.frames_for(e.T1); }
            } else {
                const int64_t F = e.flush ? m.frames_for(e.T1) : F1;
                if (F > e.E0) { runs = true; r.start = (e.E0 - g.halo_e) * g.hop; r.width = (e.flush ? e.T1 : F1 * g.hop) - r.start; r.n_new = F - e.E0; }
            }
            if (runs && !r.one_clip) {   // the window's own frame count, by the same pad plans
                bool d9 = false;
                const int64_t fw = front_frames(m, r.width, &d9);
                if (d9 || fw - r.n_new != (r.first ? 0 : g.halo_e) || r.start < 0)
                    fail(NC_ESTATE, "internal: slot %d: a window of %lld samples gives %lld frames for %lld new ones", e.id, (long long)r.width, (long long)fw, (long long)r.n_new);
            }
            e.n_out = runs ? r.n_new : 0;
        } else {
            if (e.E0 == 0) {
                if (e.T1 >= g.min_d) { runs = true; r.first = true; r.start = 0; r.width = e.T1; r.n_new = e.T1; }
                else if (e.flush) { runs = true; r.one_clip = true; r.start = 0; r.width = e.T1; r.n_new = e.T1; }
            } else if (e.n_in > 0) { runs = true; r.start = e.T0 - g.kin_d; r.width = g.kin_d + e.n_in; r.n_new = e.n_in; }
            if (runs && !r.one_clip && r.start < 0) fail(NC_ESTATE, "internal: slot %d: a decode window starts before the stream", e.id);
            e.n_out = runs ? (r.one_clip ? m.decoded_for(e.T1) : r.n_new * g.hop) : 0;
        }
        if (runs && r.one_clip) {   // what the one-clip call would raise, decided on the pad plans, with the slot's name
            try {
                int C = 0; int64_t L = 0;
                m.trace_shape(decode, r.width, m.trace_taps() - 1, &C, &L);
            } catch (const Error& err) { fail(err.code, "slot %d: %s", e.id, err.what()); }
        }
        e.n_new = runs ? r.n_new : 0;
        e.E1 = e.E0 + e.n_new;
        P.total_out += e.n_out;
        if (runs) P.rows.push_back(r);
    }
    // launch order: keys descending, entries ascending within a key; batches of at most cap_rows rows of one key
    std::stable_sort(P.rows.begin(), P.rows.end(), [](const CzRow& a, const CzRow& b) { return a.key() != b.key() ? a.key() > b.key() : a.entry < b.entry; });
    for (size_t r = 0; r < P.rows.size();) {
        size_t end = r;
        while (end < P.rows.size() && P.rows[end].key() == P.rows[r].key() && end - r < (size_t)cap_rows) ++end;
        for (size_t q = r; q < end; ++q) { P.rows[q].batch = (int)P.batches.size(); P.rows[q].row = (int)(q - r); P.e[(size_t)P.rows[q].entry].row = (int)q; }
        P.batches.push_back({r, end - r});
        r = end;
    }
    return P;
}

void report(const CzPlan& P, nc_encodec_causal_row* rows, int64_t cap, int64_t* n_rows, int64_t* n_batches, int64_t* n_out) {
    if (n_rows) *n_rows = (int64_t)P.rows.size();
    if (n_batches) *n_batches = (int64_t)P.batches.size();
    if (rows)
        for (size_t r = 0; r < P.rows.size() && (int64_t)r < cap; ++r) {
            const CzRow& w = P.rows[r];
            rows[r] = {w.entry, w.batch, w.row, w.one_clip ? 1 : 0, w.start, w.width, w.n_new};
        }
    if (n_out)
        for (size_t i = 0; i < P.e.size(); ++i) n_out[i] = P.e[i].n_out;
}

void fill_info(const CzGeom& g, nc_encodec_causal_info* info) {
    *info = {g.hop, g.halo_e, g.halo_d, g.min_e, g.min_d, g.carry_e, g.carry_d, g.taint_e, g.taint_d};
}

// the job tables of a step: every list is bounds-checked as it is written; they travel behind the descriptors of RgTables (its `extra`)
struct JobTabs {
    std::vector<std::vector<CzJob>> lists;
    std::vector<int64_t> longest;
    size_t open(void) { lists.emplace_back(); longest.push_back(1); return lists.size() - 1; }
    void add(size_t li, int64_t src, int64_t src_rs, int64_t src_elems, int64_t dst, int64_t dst_rs, int64_t dst_elems, int64_t rows, int64_t cols, int slot) {
        if (rows <= 0 || cols <= 0) return;
        if (src < 0 || dst < 0 || src_rs < cols || dst_rs < cols || src + (rows - 1) * src_rs + cols > src_elems || dst + (rows - 1) * dst_rs + cols > dst_elems)
            fail(NC_ESTATE, "internal: slot %d: a copy of %lld x %lld leaves its tensors", slot, (long long)rows, (long long)cols);
        lists[li].push_back({src, dst, src_rs, dst_rs, rows, cols});
        longest[li] = std::max(longest[li], rows * cols);
    }
    std::vector<size_t> at;   // byte offset of every list in the image
    size_t pack(std::vector<char>& img) {
        at.clear();
        for (const auto& l : lists) {
            at.push_back(img.size());
            img.resize(img.size() + l.size() * sizeof(CzJob));
            if (!l.empty()) std::memcpy(img.data() + at.back(), l.data(), l.size() * sizeof(CzJob));
        }
        return img.size();
    }
};

template <class T>
void launch_jobs(EncodecModel& m, const JobTabs& jt, const char* dimg, size_t li, const T* src, T* dst) {
    const std::vector<CzJob>& l = jt.lists[li];
    if (l.empty()) return;
    const CzJob* dj = reinterpret_cast<const CzJob*>(dimg + jt.at[li]);
    const unsigned gx = (unsigned)std::min<int64_t>(std::max<int64_t>(1, (jt.longest[li] + 1023) / 1024), 1024);
    for_grid_y(l.size(), [&](size_t done, size_t cnt) {
        double bytes = 0;
        if (m.prof.on)
            for (size_t i = 0; i < cnt; ++i) bytes += 2.0 * sizeof(T) * (double)(l[done + i].rows * l[done + i].cols);
        ProfScope ps(&m.prof, m.stream, NC_KC_ELEM, 0.0, bytes);
        hipLaunchKernelGGL(cz_copy2d_kernel<T>, dim3(gx, (unsigned)cnt), dim3(256), 0, m.stream, dj + done, src, dst);
        NC_HIP(hipGetLastError());
    });
}

// while it lives the handle's one-clip launches take the step-wise LSTM form: a causal step never launches a kernel that waits on other workgroups
struct StepwiseScope {
    LstmRuntime& r;
    bool prev;
    explicit StepwiseScope(LstmRuntime& rt) : r(rt), prev(rt.force_stepwise) { r.force_stepwise = true; }
    ~StepwiseScope() { r.force_stepwise = prev; }
};

}  // namespace

// ===================================================================================================================== the pool
struct nc_encodec_causal_pool {
    nc_codec* h = nullptr;
    bool decode = false;
    int nq = 0;                          // Decode: codebooks in the pushed codes
    CzGeom g;
    struct Slot {
        int64_t T = 0;                   // samples (Encode) or code frames (Decode) received
        int64_t E = 0;                   // frames emitted (Encode) or decoded (Decode)
        int64_t base = 0;                // position in the stream of the first element the carry holds
        bool ended = false;
        int cur = 0;                     // the half of the input carry that holds the slot's state
    };
    std::vector<Slot> slots;
    int rows_in = 0;                     // rows of the input carry: channels (Encode) | codebooks (Decode)
    int64_t cap_t = 0;                   // elements per row of a slot's half: samples | code frames
    int64_t keep = 0;                    // LSTM-output frames a slot carries: K - 1 (Encode) | halo_d (Decode)
    TwoHalves halves;                    // of the carry: [rows_in][cap_t] per slot and half
    DevBuf carry;                        // [2][n_slots][rows_in][cap_t] float PCM | int64 codes
    DevBuf arena;                        // the gathered windows of every batch of a step
    DevBuf hs, cs;                       // [n_slots][layers][Cl]
    DevBuf tail;                         // [n_slots][Cl][keep]
    DevBuf in_stage, out_stage, emb_stage;   // the packed tensors of a host-pointer call

    EncodecModel& model() const { return as<EncodecModel>(h); }
    Lstm& lstm_of(EncodecModel& m) const { return decode ? m.dec_lstm : m.enc_lstm; }
    int64_t n_slots() const { return (int64_t)slots.size(); }
    static constexpr const char* kNull = "null causal pool";
    static constexpr const char* kRange = kSlotOutOfRange;
    static constexpr int kRangeLast = 0;

    CzPlan plan(int n, const int32_t* ids, const int64_t* n_in, const int32_t* flush, const char* what) const;
    template <class T>
    void step_dev(const CzPlan& P, const T* in, void* out, float* emb);
    void run_encode(EncodecModel& m, const CzPlan& P, const CzBatch& bt, const float* x, const int32_t* d_idx, const JobTabs& jt, const char* dimg, const size_t* jl,
                    const RgTables& t, size_t li, int64_t* codes, float* emb);
    void run_decode(EncodecModel& m, const CzPlan& P, const CzBatch& bt, const int64_t* cw, const int32_t* d_idx, const JobTabs& jt, const char* dimg, const size_t* jl,
                    const RgTables& t, size_t li, float* pcm);
    void commit(const CzPlan& P);
};

// every refusal that needs the slots' state, then the plan (which refuses the rest); nothing is changed
CzPlan nc_encodec_causal_pool::plan(int n, const int32_t* ids, const int64_t* n_in, const int32_t* flush, const char* what) const {
    std::vector<int64_t> T0, E0;
    pool_named_slots(*this, n, ids, n_in, what, &Slot::E, T0, E0);
    const EncodecModel& m = model();
    return make_plan(m, g, decode, n, ids, T0.data(), E0.data(), n_in, flush, m.ragged_rows, what);
}

void nc_encodec_causal_pool::commit(const CzPlan& P) {
    for (const CzEntry& e : P.e) {
        Slot& s = slots[(size_t)e.id];
        s.T = e.T1; s.E = e.E1;
        if (e.flush) { s.ended = true; continue; }
        if (e.row >= 0) {   // the step rewrote the carry into the other half
            s.cur ^= 1;
            s.base = decode ? std::max<int64_t>(0, e.T1 - g.carry_d) : std::max<int64_t>(0, e.E1 - g.halo_e) * g.hop;
        }
    }
}

// One step on device pointers.  T = float (Encode: PCM in) | int64_t (Decode: codes in).
template <class T>
void nc_encodec_causal_pool::step_dev(const CzPlan& P, const T* in, void* out, float* emb) {
    EncodecModel& m = model();
    m.use_device();
    m.check_async_errors();   // an earlier device-pointer call on this handle may have timed out unnoticed
    m.pool_i = 0;
    const int R = rows_in, D = m.cfg.dimension, Cl = lstm_of(m).C, Cn = m.cfg.channels, nqe = m.n_q;
    const int64_t in_elems = (int64_t)R * P.total_in;
    // the batches' gathered windows in the arena
    std::vector<int64_t> x_off;
    int64_t x_total = 0;
    for (const CzBatch& bt : P.batches) { x_off.push_back(x_total); x_total += round_up((int64_t)bt.count * R * P.rows[bt.first].width, kAlign); }
    JobTabs jt;
    const size_t j_ca = jt.open(), j_ia = jt.open(), j_cc = jt.open(), j_ic = jt.open();   // carry -> arena, in -> arena, carry -> carry, in -> carry
    // [g0, g0 + len) of entry e's stream to dst (row pitch dst_rs): [base, T0) sits in the slot's current half, [T0, T1) in the entry's input
    auto gather = [&](const CzEntry& e, int64_t g0, int64_t len, bool to_carry, int64_t dst, int64_t dst_rs, int64_t dst_elems) {
        const Slot& s = slots[(size_t)e.id];
        const int64_t a_n = std::min(len, std::max<int64_t>(0, e.T0 - g0)), b_n = len - a_n;
        if (len < 0 || g0 < s.base || g0 + len > e.T1 || e.T0 - s.base > cap_t) fail(NC_ESTATE, "internal: slot %d: a window leaves what the slot holds", e.id);
        jt.add(to_carry ? j_cc : j_ca, halves.at(s.cur, e.id) + (g0 - s.base), cap_t, halves.elems(), dst, dst_rs, dst_elems, R, a_n, e.id);
        jt.add(to_carry ? j_ic : j_ia, (int64_t)R * e.in_off + (g0 + a_n - e.T0), e.n_in, in_elems, dst + a_n, dst_rs, dst_elems, R, b_n, e.id);
    };
    for (size_t bi = 0; bi < P.batches.size(); ++bi)
        for (size_t r = 0; r < P.batches[bi].count; ++r) {
            const CzRow& w = P.rows[P.batches[bi].first + r];
            gather(P.e[(size_t)w.entry], w.start, w.width, false, x_off[bi] + (int64_t)r * R * w.width, w.width, x_total);
        }
    for (const CzEntry& e : P.e) {
        if (e.flush) continue;
        const Slot& s = slots[(size_t)e.id];
        if (e.row >= 0) {        // frames went out: what the next step needs, into the other half
            const int64_t base1 = decode ? std::max<int64_t>(0, e.T1 - g.carry_d) : std::max<int64_t>(0, e.E1 - g.halo_e) * g.hop;
            if (e.T1 - base1 > cap_t) fail(NC_ESTATE, "internal: slot %d keeps more than its carry holds", e.id);
            gather(e, base1, e.T1 - base1, true, halves.at(s.cur ^ 1, e.id), cap_t, halves.elems());
        } else if (e.n_in > 0) { // nothing went out: the push is appended behind what the slot holds
            if (e.T1 - s.base > cap_t) fail(NC_ESTATE, "internal: slot %d holds more than its carry", e.id);
            gather(e, e.T0, e.n_in, true, halves.at(s.cur, e.id) + (e.T0 - s.base), cap_t, halves.elems());
        }
    }
    // per batch: the rows' slots, the concatenation of carried and new LSTM frames, the new carry, the emission
    RgTables t;
    std::vector<size_t> first_launch, first_job, idx_at;
    std::vector<int32_t> idx;
    const int64_t tail_elems = n_slots() * Cl * keep;
    for (const CzBatch& bt : P.batches) {
        const CzRow& k = P.rows[bt.first];
        const int64_t N = (int64_t)bt.count, n = k.n_new, kc = k.first ? 0 : keep, W = kc + n;
        first_launch.push_back(t.launches.size());
        first_job.push_back(jt.lists.size());
        idx_at.push_back(idx.size());
        const size_t j_tz = jt.open(), j_yz = jt.open(), j_zt = jt.open();   // tail -> z, y -> z, z -> tail
        for (int64_t r = 0; r < N; ++r) {
            const CzEntry& e = P.e[(size_t)P.rows[bt.first + (size_t)r].entry];
            idx.push_back(e.id); idx.push_back(k.first ? 1 : 0);
            if (k.one_clip) continue;
            if (n + kc < keep) fail(NC_ESTATE, "internal: slot %d: fewer LSTM frames than the slot carries", e.id);
            jt.add(j_tz, (int64_t)e.id * Cl * keep, keep, tail_elems, r * Cl * W, W, N * Cl * W, Cl, kc, e.id);
            jt.add(j_yz, r * Cl * n, n, N * Cl * n, r * Cl * W + kc, W, N * Cl * W, Cl, n, e.id);
            if (!e.flush) jt.add(j_zt, r * Cl * W + (W - keep), W, N * Cl * W, (int64_t)e.id * Cl * keep, keep, tail_elems, Cl, keep, e.id);
        }
        if (!decode) {
            t.begin(N * nqe * n, nqe * P.total_out);
            for (int64_t r = 0; r < N; ++r) t.add(r * nqe * n, nqe * P.e[(size_t)P.rows[bt.first + (size_t)r].entry].out_off, nqe * n);
            t.end();
            if (emb) {
                t.begin(N * D * n, D * P.total_out);
                for (int64_t r = 0; r < N; ++r) t.add(r * D * n, D * P.e[(size_t)P.rows[bt.first + (size_t)r].entry].out_off, D * n);
                t.end();
            }
        } else {
            const int64_t Lo = P.e[(size_t)k.entry].n_out;
            t.begin(N * Cn * Lo, Cn * P.total_out);
            for (int64_t r = 0; r < N; ++r) t.add(r * Cn * Lo, Cn * P.e[(size_t)P.rows[bt.first + (size_t)r].entry].out_off, Cn * Lo);
            t.end();
        }
    }
    bool any = false;
    for (const auto& l : jt.lists) any = any || !l.empty();
    if (!any && P.batches.empty()) return;   // (entries that push nothing and flush nothing)
    const size_t jobs_bytes = jt.pack(t.extra);
    t.extra.resize(jobs_bytes + std::max<size_t>(8, (idx.size() * 4 + 7) / 8 * 8));
    if (!idx.empty()) std::memcpy(t.extra.data() + jobs_bytes, idx.data(), idx.size() * 4);
    arena.reserve((size_t)std::max<int64_t>(x_total, 4) * sizeof(T));
    const char* dimg = rg_upload(m, t);
    const int32_t* d_idx = reinterpret_cast<const int32_t*>(dimg + jobs_bytes);
    launch_jobs<T>(m, jt, dimg, j_ca, carry.as<T>(), arena.as<T>());
    launch_jobs<T>(m, jt, dimg, j_ia, in, arena.as<T>());
    launch_jobs<T>(m, jt, dimg, j_cc, carry.as<T>(), carry.as<T>());
    launch_jobs<T>(m, jt, dimg, j_ic, in, carry.as<T>());
    StepwiseScope stepwise(m.lstm);
    for (size_t bi = 0; bi < P.batches.size(); ++bi) {
        const size_t jl[3] = {first_job[bi], first_job[bi] + 1, first_job[bi] + 2};
        if constexpr (std::is_same<T, float>::value)
            run_encode(m, P, P.batches[bi], arena.as<float>() + x_off[bi], d_idx + idx_at[bi], jt, dimg, jl, t, first_launch[bi], static_cast<int64_t*>(out), emb);
        else
            run_decode(m, P, P.batches[bi], arena.as<int64_t>() + x_off[bi], d_idx + idx_at[bi], jt, dimg, jl, t, first_launch[bi], static_cast<float*>(out));
    }
}

// ===================================================================================================================== Encode
// One batch of N windows [N, channels, width]: front -> drop the halo -> carried LSTM on the new frames -> last convolution on
// [carried K - 1 frames + new] -> drop the carried part -> quantizer.  (Encodec.Encode -> EncodeFrame -> SEANetEncoder.forward)
void nc_encodec_causal_pool::run_encode(EncodecModel& m, const CzPlan& P, const CzBatch& bt, const float* x, const int32_t* d_idx, const JobTabs& jt,
                                        const char* dimg, const size_t* jl, const RgTables& t, size_t li, int64_t* codes, float* emb) {
    const CzRow& k = P.rows[bt.first];
    const int N = (int)bt.count, D = m.cfg.dimension, nqe = m.n_q;
    const int64_t n = k.n_new;
    int64_t* cb = reinterpret_cast<int64_t*>(m.alloc((size_t)N * nqe * n * 2));
    float* residual = nullptr;
    if (k.one_clip) {   // a stream flushed below the minimum: the one-clip call on what it holds
        float* eb = m.alloc((size_t)N * D * n);
        m.encode_batch(x, N, k.width, n, cb, nullptr, eb);
        rg_copy_i64(m, t, li++, cb, codes);
        if (emb) rg_copy_f32(m, t, li++, eb, emb);
        return;
    }
    EncodecModel::Act a;
    a.p = x; a.C = m.cfg.channels; a.L = k.width; a.rs = k.width; a.off = 0;
    EncodecModel::Act f = m.encoder_front(a, N);
    const int64_t drop = f.L - n;
    if (drop != (k.first ? 0 : g.halo_e)) fail(NC_ESTATE, "internal: the front produced %lld frames for %lld new ones", (long long)f.L, (long long)n);
    f.off += drop; f.L = n;
    const float* xl = m.materialize(f, N, nullptr, 0);
    const bool lstm_elu = lstm_applies_elu(m.enc_lstm);
    const int Cl = f.C;
    const float* y = m.enc_lstm.layers.empty() ? xl : lstm_run_carried(m, m.enc_lstm, xl, N, n, lstm_elu, d_idx, hs.as<float>(), cs.as<float>());
    const int64_t kc = k.first ? 0 : keep, W = kc + n;
    const float* z = y;
    if (kc > 0) {
        float* zz = m.alloc((size_t)N * Cl * W);
        launch_jobs<float>(m, jt, dimg, jl[0], tail.as<float>(), zz);
        launch_jobs<float>(m, jt, dimg, jl[1], y, zz);
        z = zz;
    }
    launch_jobs<float>(m, jt, dimg, jl[2], z, tail.as<float>());
    EncodecModel::Act za;
    za.p = z; za.C = Cl; za.L = W; za.rs = W; za.off = 0;
    EncodecModel::Act e = m.sconv(m.enc_out, za, nullptr, !lstm_elu, N);
    if (e.L != W) fail(NC_ESTATE, "internal: the last convolution produced %lld frames of %lld", (long long)e.L, (long long)W);
    e.off += kc; e.L = n;
    residual = m.materialize(e, N, nullptr, 0);
    if (emb) rg_copy_f32(m, t, li + 1, residual, emb);
    if (m.prof.on) m.prof.begin(m.stream, NC_KC_RVQ, 2.0 * D * m.cfg.codebook_size * (double)N * n * nqe, 0.0);
    launch_euclid_rvq(m.book_tab, nqe, -1, residual, N, n, cb, m.stream);
    if (m.prof.on) m.prof.end(m.stream);
    rg_copy_i64(m, t, li, cb, codes);
}

// ===================================================================================================================== Decode
// One batch of N code windows [N, n_q, width]: embedding sum -> first convolution on [carried K - 1 frames + new] -> drop the carried part
// -> carried LSTM on the new frames -> up-stack and last convolution on [carried halo_d LSTM frames + new] -> the last n * hop samples.
// (Encodec.Decode -> DecodeFrame -> SEANetDecoder.forward)
void nc_encodec_causal_pool::run_decode(EncodecModel& m, const CzPlan& P, const CzBatch& bt, const int64_t* cw, const int32_t* d_idx, const JobTabs& jt,
                                        const char* dimg, const size_t* jl, const RgTables& t, size_t li, float* pcm) {
    const CzRow& k = P.rows[bt.first];
    const int N = (int)bt.count, D = m.cfg.dimension;
    const int64_t n = k.n_new, Lo_want = P.e[(size_t)k.entry].n_out;
    if (k.one_clip) {
        int64_t Lo = 0;
        const float* o = m.decode_batch(cw, N, nq, k.width, nullptr, &Lo);
        if (Lo != Lo_want) fail(NC_ESTATE, "internal: decoder produced %lld samples, planned %lld", (long long)Lo, (long long)Lo_want);
        rg_copy_f32(m, t, li, o, pcm);
        return;
    }
    float* eb = m.alloc((size_t)N * D * k.width);
    launch_emb_sum(m.book_tab, cw, nq, N, k.width, eb, m.stream);
    EncodecModel::Act a;
    a.p = eb; a.C = D; a.L = k.width; a.rs = k.width; a.off = 0;
    EncodecModel::Act f = m.sconv(m.dec_in, a, nullptr, false, N);
    const int64_t drop = f.L - n;
    if (drop != (k.first ? 0 : g.kin_d)) fail(NC_ESTATE, "internal: the first convolution produced %lld frames for %lld new ones", (long long)f.L, (long long)n);
    f.off += drop; f.L = n;
    const float* xl = m.materialize(f, N, nullptr, 0);
    const bool lstm_elu = lstm_applies_elu(m.dec_lstm);
    const int Cl = f.C;
    const float* y = m.dec_lstm.layers.empty() ? xl : lstm_run_carried(m, m.dec_lstm, xl, N, n, lstm_elu, d_idx, hs.as<float>(), cs.as<float>());
    const int64_t kc = k.first ? 0 : keep, W = kc + n;
    const float* z = y;
    if (kc > 0) {
        float* zz = m.alloc((size_t)N * Cl * W);
        launch_jobs<float>(m, jt, dimg, jl[0], tail.as<float>(), zz);
        launch_jobs<float>(m, jt, dimg, jl[1], y, zz);
        z = zz;
    }
    launch_jobs<float>(m, jt, dimg, jl[2], z, tail.as<float>());
    EncodecModel::Act za;
    za.p = z; za.C = Cl; za.L = W; za.rs = W; za.off = 0;
    EncodecModel::Act o = m.decoder_tail(za, lstm_elu, N);
    if (o.L != W * g.hop || Lo_want != n * g.hop) fail(NC_ESTATE, "internal: the up-stack produced %lld samples of %lld frames", (long long)o.L, (long long)W);
    o.off += kc * g.hop; o.L = n * g.hop;
    rg_copy_f32(m, t, li, m.materialize(o, N, nullptr, 0), pcm);
}

// ================================================================================================ C ABI
namespace {

void pool_step(nc_encodec_causal_pool& x, bool host, int32_t n, const int32_t* slots, const int64_t* n_in, const int32_t* flush, const void* in, void* out, float* emb,
               int64_t out_cap, int64_t* n_out) {
    const char* what = host ? "nc_encodec_causal_pool_step" : "nc_encodec_causal_pool_step_dev";
    EncodecModel& m = x.model();
    const CzPlan P = x.plan(n, slots, n_in, flush, what);
    if (!m.loaded) fail(NC_ESTATE, "weights not loaded (call nc_codec_load_weights first)");
    const int64_t need = (x.decode ? (int64_t)m.cfg.channels : (int64_t)m.n_q) * P.total_out;
    if (out_cap < need) fail(NC_EINVAL, "%s: out_cap is %lld, the step writes %lld elements (nc_encodec_causal_pool_query)", what, (long long)out_cap, (long long)need);
    if ((P.total_in > 0 && !in) || (need > 0 && !out)) fail(NC_EINVAL, "%s: null pointer", what);
    if (!host) { m.use_device(); m.check_async_errors(); }   // (an earlier call's failure: reported before this step touches anything)
    // From here on the step writes the slots' device state (carry halves, (h, c), LSTM frames).  A failure past this point -- a HIP error,
    // an internal check -- leaves that state of the named slots undefined while their counters are uncommitted: they are ended, so the
    // next push to one of them is refused until nc_encodec_causal_pool_reset_slot starts a new stream.  Slots not named are untouched.
    struct EndOnFailure {
        nc_encodec_causal_pool& x;
        const CzPlan& P;
        bool armed = true;
        ~EndOnFailure() {
            if (armed)
                for (const CzEntry& e : P.e) x.slots[(size_t)e.id].ended = true;
        }
    } on_failure{x, P};
    if (!host) {
        if (x.decode) x.step_dev<int64_t>(P, static_cast<const int64_t*>(in), out, nullptr);
        else x.step_dev<float>(P, static_cast<const float*>(in), out, emb);
    } else {
        OwnStreamScope own(m);
        m.lstm.note_timeout();   // (left behind by an earlier device-pointer call: not this call's failure; a causal step launches no kernel that can time out)
        if (x.decode)
            pool_step_staged(x, m.stream, in, (size_t)x.nq * P.total_in * 8, out, (size_t)need * 4, nullptr, 0,
                             [&](void* din, void* dout, float*) { x.step_dev<int64_t>(P, static_cast<const int64_t*>(din), dout, nullptr); });
        else
            pool_step_staged(x, m.stream, in, (size_t)m.cfg.channels * P.total_in * 4, out, (size_t)need * 8, emb, (size_t)m.cfg.dimension * P.total_out * 4,
                             [&](void* din, void* dout, float* demb) { x.step_dev<float>(P, static_cast<const float*>(din), dout, demb); });
    }
    on_failure.armed = false;
    x.commit(P);
    if (n_out)
        for (size_t i = 0; i < P.e.size(); ++i) n_out[i] = P.e[i].n_out;
}

}  // namespace

extern "C" {

nc_status nc_encodec_causal_plan(const nc_encodec_config* cfg, int32_t decode, int32_t n, const int64_t* received, const int64_t* emitted, const int64_t* n_in,
                                 const int32_t* flush, int32_t max_rows, nc_encodec_causal_info* info, nc_encodec_causal_row* rows, int64_t cap, int64_t* n_rows,
                                 int64_t* n_batches, int64_t* n_out) {
    return guard([&] {
        const char* what = "nc_encodec_causal_plan";
        if (!cfg) fail(NC_EINVAL, "cfg must not be null");
        const EncodecModel m(*cfg);   // host arithmetic alone: no device is touched
        const CzGeom g = geom_of(m, what);
        if (info) fill_info(g, info);
        if (!received || !emitted || !n_in) fail(NC_EINVAL, "%s: null pointer", what);
        if (n <= 0) fail(NC_EINVAL, "%s: n must be positive", what);
        for (int i = 0; i < n; ++i) {   // the position of a stream that has not been flushed follows from what it has received
            if (received[i] < 0) fail(NC_EINVAL, "%s: stream %d: received is negative", what, i);
            const int64_t f = decode ? received[i] : received[i] / g.hop;
            const int64_t want = f >= (decode ? g.min_d : g.min_e) ? f : 0;
            if (emitted[i] != want)
                fail(NC_EINVAL, "%s: stream %d: a stream that has received %lld has emitted %lld, not %lld", what, i, (long long)received[i], (long long)want, (long long)emitted[i]);
        }
        report(make_plan(m, g, decode != 0, n, nullptr, received, emitted, n_in, flush, max_rows, what), rows, cap, n_rows, n_batches, n_out);
    });
}

nc_status nc_encodec_causal_pool_create(nc_codec* h, int32_t decode, int32_t n_slots, int32_t n_q, nc_encodec_causal_pool** out) {
    return guard([&] {
        if (!out) fail(NC_EINVAL, "out must not be null");
        *out = nullptr;
        EncodecModel& m = as<EncodecModel>(h);
        std::unique_ptr<nc_encodec_causal_pool> p(new nc_encodec_causal_pool);
        p->h = h;
        p->decode = decode != 0;
        p->g = geom_of(m, "nc_encodec_causal_pool_create");
        if (n_slots <= 0 || n_slots > 65536) fail(NC_EINVAL, "n_slots must be in 1..65536");
        if (n_q < 0 || n_q > m.cfg.n_codebooks) fail(NC_EINVAL, "codes carry %d codebooks; the model has %d", n_q, m.cfg.n_codebooks);
        p->nq = n_q > 0 ? n_q : m.n_q;
        p->slots.resize((size_t)n_slots);
        const CzGeom& g = p->g;
        p->rows_in = p->decode ? p->nq : m.cfg.channels;
        p->cap_t = p->decode ? g.carry_d : std::max(g.min_e, g.halo_e + 1) * g.hop;
        p->halves = {n_slots, (int64_t)p->rows_in * p->cap_t};
        p->keep = p->decode ? g.halo_d : g.carry_e;
        const int Cl = m.cfg.n_filters << m.cfg.n_ratios, nl = std::max(1, m.cfg.lstm_layers);
        m.use_device();
        p->carry.reserve((size_t)std::max<int64_t>(p->halves.elems(), 4) * (p->decode ? 8 : 4));
        p->hs.reserve((size_t)n_slots * nl * Cl * 4);
        p->cs.reserve((size_t)n_slots * nl * Cl * 4);
        p->tail.reserve((size_t)std::max<int64_t>((int64_t)n_slots * Cl * p->keep, 4) * 4);
        *out = p.release();
    });
}

nc_status nc_encodec_causal_pool_destroy(nc_encodec_causal_pool* p) {
    return guard([&] { delete p; });
}

nc_status nc_encodec_causal_pool_reset_slot(nc_encodec_causal_pool* p, int32_t slot) {
    return guard([&] {
        reset_keep_cur(slot_of(pool_of(p), slot));
    });
}

nc_status nc_encodec_causal_pool_pending(const nc_encodec_causal_pool* p, int32_t slot, int64_t* n) {
    return guard([&] {
        if (!n) fail(NC_EINVAL, "n must not be null");
        nc_encodec_causal_pool& x = pool_of(p);
        const nc_encodec_causal_pool::Slot& s = slot_of(x, slot);
        if (s.ended) *n = 0;
        else if (x.decode) *n = s.T - s.E;
        else *n = s.T - s.E * x.g.hop;
    });
}

nc_status nc_encodec_causal_pool_query(const nc_encodec_causal_pool* p, int32_t n, const int32_t* slots, const int64_t* n_in, const int32_t* flush, int64_t* n_out) {
    return guard([&] {
        nc_encodec_causal_pool& x = pool_of(p);
        report(x.plan(n, slots, n_in, flush, "nc_encodec_causal_pool_query"), nullptr, 0, nullptr, nullptr, n_out);
    });
}

nc_status nc_encodec_causal_pool_plan(const nc_encodec_causal_pool* p, int32_t n, const int32_t* slots, const int64_t* n_in, const int32_t* flush,
                                      nc_encodec_causal_row* rows, int64_t cap, int64_t* n_rows, int64_t* n_batches) {
    return guard([&] {
        nc_encodec_causal_pool& x = pool_of(p);
        report(x.plan(n, slots, n_in, flush, "nc_encodec_causal_pool_plan"), rows, cap, n_rows, n_batches, nullptr);
    });
}

nc_status nc_encodec_causal_pool_step(nc_encodec_causal_pool* p, int32_t n, const int32_t* slots, const int64_t* n_in, const int32_t* flush, const void* in_packed,
                                      void* out_packed, float* emb_packed, int64_t out_cap, int64_t* n_out) {
    return guard([&] { pool_step(pool_of(p), true, n, slots, n_in, flush, in_packed, out_packed, emb_packed, out_cap, n_out); });
}

nc_status nc_encodec_causal_pool_step_dev(nc_encodec_causal_pool* p, int32_t n, const int32_t* slots, const int64_t* n_in, const int32_t* flush, const void* in_packed,
                                          void* out_packed, float* emb_packed, int64_t out_cap, int64_t* n_out) {
    return guard([&] { pool_step(pool_of(p), false, n, slots, n_in, flush, in_packed, out_packed, emb_packed, out_cap, n_out); });
}

// test hook: one SLSTM stack from given state through lstm_run_carried (row b's state lives in slot b)
nc_status nc_op_encodec_lstm_carried(nc_codec* h, int32_t decoder, const float* x, int32_t N, int64_t T, float* h_state, float* c_state, float* y) {
    return guard([&] {
        EncodecModel& m = as<EncodecModel>(h);
        if (!m.loaded) fail(NC_ESTATE, "weights not loaded (call nc_codec_load_weights first)");
        Lstm& l = decoder ? m.dec_lstm : m.enc_lstm;
        if (!x || !y || (h_state == nullptr) != (c_state == nullptr)) fail(NC_EINVAL, "x and y must be given, h_state and c_state together");
        if (N <= 0 || N > 4096 || T <= 0 || T > ((int64_t)1 << 20) || l.layers.empty()) fail(NC_EINVAL, "N in 1..4096, T in 1..2^20, and the model must have an LSTM");
        const int C = l.C, nl = (int)l.layers.size();
        const size_t n_x = (size_t)N * C * T * 4, n_s = (size_t)N * nl * C * 4;
        OwnStreamScope own(m);
        m.pool_i = 0;
        DevBuf dx, dh, dc, di;
        dx.reserve(n_x); dh.reserve(n_s); dc.reserve(n_s); di.reserve((size_t)N * 8);
        std::vector<int32_t> idx((size_t)2 * N);
        for (int b = 0; b < N; ++b) { idx[(size_t)2 * b] = b; idx[(size_t)2 * b + 1] = h_state ? 0 : 1; }
        NC_HIP(hipMemcpyAsync(dx.p, x, n_x, hipMemcpyHostToDevice, m.stream));
        NC_HIP(hipMemcpyAsync(di.p, idx.data(), (size_t)N * 8, hipMemcpyHostToDevice, m.stream));
        if (h_state) {
            NC_HIP(hipMemcpyAsync(dh.p, h_state, n_s, hipMemcpyHostToDevice, m.stream));
            NC_HIP(hipMemcpyAsync(dc.p, c_state, n_s, hipMemcpyHostToDevice, m.stream));
        }
        const float* out = lstm_run_carried(m, l, dx.as<float>(), N, T, lstm_applies_elu(l), di.as<int32_t>(), dh.as<float>(), dc.as<float>());
        NC_HIP(hipMemcpyAsync(y, out, n_x, hipMemcpyDeviceToHost, m.stream));
        if (h_state) {
            NC_HIP(hipMemcpyAsync(h_state, dh.p, n_s, hipMemcpyDeviceToHost, m.stream));
            NC_HIP(hipMemcpyAsync(c_state, dc.p, n_s, hipMemcpyDeviceToHost, m.stream));
        }
        NC_HIP(hipStreamSynchronize(m.stream));
    });
}

}  // extern "C"
