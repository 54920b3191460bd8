// What the pooled Encodec drivers share (nc_encodec_ragged.hip: the segments of whole clips; nc_encodec_stream.hip: the segments of live
// streams): a row is one (clip | stream, segment) pair, rows of equal key form batches, every batch goes to a lane -- and the arithmetic
// of DSP.LinearOverlapAdd for one output sample, which both overlap-add kernels compile from this one definition under the unit's
// contraction setting (-ffp-contract=off).
#pragma once
#include <algorithm>
#include <cmath>
#include <map>
#include <string>
#include <vector>

#include "nc_model.h"

namespace nc {

// the best measured value of profiles/encodec_ragged_bench.json
constexpr int32_t kDefaultRaggedRows = 128;
// rows per batch for a max_rows setting (0: the default); NC_EINVAL outside 0 .. RAGGED_MAX_ROWS
inline int64_t er_max_rows(int32_t max_rows, const char* what) {
    if (max_rows < 0 || max_rows > EncodecModel::RAGGED_MAX_ROWS)
        fail(NC_EINVAL, "%s: max_rows must be 0 (default) .. %d", what, EncodecModel::RAGGED_MAX_ROWS);
    return max_rows > 0 ? max_rows : kDefaultRaggedRows;
}

// ---- overlap-add ---------------------------------------------------------------------------------------------------------------------
struct OlaClip {             // one (clip, channel) of the output
    int64_t out, total;      // first element in pcm_packed, samples
    int64_t first;           // the clip's frame 0 in the frame table
    int64_t L0;              // length of frame 0: the clip's window (a clip shorter than a segment has its own)
    int32_t nfr, ch;
    float eps;               // AudioTensorDSP.cs:246-252: 1e-10f where some weight sum is <= 1e-10f, else 0
    int32_t pad_;
};
struct OlaFrame { int64_t off, len, pitch; };   // rows [channels] of `len` samples, `pitch` elements apart, of a decoded frame (elements from the frames' base)

#ifdef __HIPCC__
// DSP.LinearOverlapAdd for sample t of one (clip, channel): the arithmetic of ola_tables + overlap_add_kernel (nc_encodec.hip), operation
// for operation -- w[q] = 0.5f - |(float)((q + 1) / (double)(L0 + 1)) - 0.5f|, the weight sum added up in fp32 in ascending frame order
// from 0.0f, a = a + x * w in the same order, one division.  Only the frames that can cover t are visited: the others add nothing on the
// host either (no frame is longer than the first, checked before the launch).
__device__ __forceinline__ float ola_sample(const OlaClip& d, const OlaFrame* __restrict__ fr, const float* __restrict__ frames, int64_t stride, int64_t t) {
    const int64_t f_lo = t >= d.L0 ? (t - d.L0) / stride + 1 : 0;
    const int64_t f_hi = min((int64_t)d.nfr - 1, t / stride);
    const double den = (double)(d.L0 + 1);
    float a = 0.0f, sw = 0.0f;
    for (int64_t f = f_lo; f <= f_hi; ++f) {
        const OlaFrame g = fr[d.first + f];
        const int64_t q = t - f * stride;
        if (q >= 0 && q < g.len) {
            const float tt = (float)((double)(q + 1) / den);
            const float w = 0.5f - fabsf(tt - 0.5f);
            a = a + frames[g.off + (int64_t)d.ch * g.pitch + q] * w;
            sw = sw + w;
        }
    }
    return a / (sw + d.eps);   // (eps = 0: sw + 0.0f is sw)
}
#endif

// The host's `+ 1e-10` branch (ola_tables): taken when some weight sum is <= 1e-10f.  The window is unimodal (t rises with i and both
// roundings are monotone), so every value is >= the smaller of its two ends; where every sample is covered (no frame but the last is
// shorter than the stride) a weight sum is a sum of at least one such value.  Only where that bound does not decide it -- windows of
// more than 2^25 samples, whose ends round to zero, or frames that leave gaps -- are the sums added up as the host does.
inline float ola_eps(const std::vector<int64_t>& flen, int64_t stride, int64_t total) {
    const int64_t L0 = flen[0];
    auto w = [&](int64_t i) {
        const float t = (float)((double)(i + 1) / (double)(L0 + 1));
        return 0.5f - std::fabs(t - 0.5f);
    };
    bool covered = true;
    for (size_t f = 0; f + 1 < flen.size(); ++f) covered = covered && flen[f] >= stride;
    if (covered && std::min(w(0), w(L0 - 1)) > 1e-10f) return 0.0f;
    std::vector<float> sw((size_t)total, 0.0f);
    for (size_t f = 0; f < flen.size(); ++f)
        for (int64_t i = 0; i < flen[f]; ++i) sw[(size_t)((int64_t)f * stride + i)] = sw[(size_t)((int64_t)f * stride + i)] + w(i);
    float mn = INFINITY;
    for (float v : sw) mn = std::min(mn, v);
    return mn <= 1e-10f ? 1e-10f : 0.0f;
}

// ---- rows, batches, lanes ----------------------------------------------------------------------------------------------------------
struct ErRow { int32_t clip, seg; int64_t off, len, frames, key; };   // clip: the clip of a ragged call | the entry of a stream step
struct ErBatch { int64_t key; size_t first, count; };

// Launch order: keys descending, the rows of a key segment-major and then by clip; batches of at most max_rows rows of one key.
// Returns the number of distinct keys.
inline int64_t er_batches(std::vector<ErRow>& rows, int64_t max_rows, std::vector<ErBatch>& batches) {
    std::stable_sort(rows.begin(), rows.end(), [](const ErRow& a, const ErRow& b) {
        if (a.key != b.key) return a.key > b.key;
        if (a.seg != b.seg) return a.seg < b.seg;
        return a.clip < b.clip;
    });
    int64_t n_keys = 0;
    for (size_t r = 0; r < rows.size();) {
        size_t e = r;
        while (e < rows.size() && rows[e].key == rows[r].key) ++e;
        ++n_keys;
        for (; r < e; r += (size_t)max_rows) batches.push_back({rows[r].key, r, std::min<size_t>((size_t)max_rows, e - r)});
        r = e;
    }
    return n_keys;
}

// What the stacks would raise on a row ("segment too short": a residual block whose branch outgrows its shortcut), decided on the pad
// plans alone, per distinct key; the first clip in index order that holds such a row is named (ids: the name of clip i, null: i itself).
inline void er_check_rows(const EncodecModel& m, const std::vector<ErRow>& rows, bool decode, const char* noun, const int32_t* ids) {
    std::map<int64_t, std::pair<nc_status, std::string>> verdict;
    int bad_clip = -1;
    const std::pair<nc_status, std::string>* bad = nullptr;
    for (const ErRow& w : rows) {
        auto it = verdict.find(w.key);
        if (it == verdict.end()) {
            std::pair<nc_status, std::string> v{NC_OK, std::string()};
            try {
                int C = 0; int64_t L = 0;
                m.trace_shape(decode, w.key, m.trace_taps() - 1, &C, &L);
                if (decode && L != w.len) fail(NC_ESTATE, "internal: %lld frames decode to %lld samples, planned %lld", (long long)w.key, (long long)L, (long long)w.len);
            } catch (const Error& e) { v = {e.code, e.what()}; }
            it = verdict.emplace(w.key, v).first;
        }
        if (it->second.first != NC_OK && (bad_clip < 0 || w.clip < bad_clip)) { bad_clip = w.clip; bad = &it->second; }
    }
    if (bad) fail(bad->first, "%s %d: %s", noun, ids ? ids[bad_clip] : bad_clip, bad->second.c_str());
}

// Lanes: every batch goes to the stream with the least work so far, the work of a batch being its dependent LSTM steps (the chain the
// call is bound by; a launch of the persistent kernel holds 32 rows) -- the first, largest batch lands on the handle's stream.
inline std::vector<int> er_assign_lanes(const std::vector<ErRow>& rows, const std::vector<ErBatch>& batches) {
    static const bool no_overlap = env_flag("NC_ENCODEC_NO_OVERLAP");
    std::vector<int> lanes;
    int64_t load[3] = {0, 0, 0};
    for (const ErBatch& b : batches) {
        int l = 0;
        if (!no_overlap)
            for (int i = 1; i < 3; ++i)
                if (load[i] < load[l]) l = i;
        load[l] += rows[b.first].frames * (int64_t)((b.count + 31) / 32) + 8;
        lanes.push_back(l);
    }
    return lanes;
}

struct LaneScope {   // the pool in three lanes for the length of a pooled call
    EncodecModel& m;
    explicit LaneScope(EncodecModel& m_) : m(m_) { m.pool_lanes = 3; m.pool_lane = 0; m.pool_i = 0; }
    ~LaneScope() { m.pool_lanes = 1; m.pool_lane = 0; m.pool_i = 0; }
};

// A host-pointer call on the handle's own stream, as encodec_host_call of nc_api.hip: a persistent-LSTM timeout left behind by an earlier
// device-pointer call is noted and is not this call's failure; a timeout of this call's own switches the handle to the step-wise kernels
// and the launches run once more (so `run` must be repeatable: it changes nothing that it reads).
template <class Run>
void encodec_host_run(EncodecModel& m, Run&& run) {
    m.lstm.note_timeout();
    for (int attempt = 0;; ++attempt) {
        run();
        NC_HIP(hipStreamSynchronize(m.stream));
        if (!m.lstm.timed_out() || attempt) break;
        try { m.check_async_errors(); } catch (const Error&) {}
    }
    m.check_async_errors();
}

}  // namespace nc
