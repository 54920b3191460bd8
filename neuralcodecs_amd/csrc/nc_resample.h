// Band-limited resampling (include/nc_mi355x.h "band-limited resampling"): what the device unit (nc_resample.hip) and the
// serial host twin (nc_resample_host.hip) share -- the argument checks, the geometry and the table builder.  Nothing of the arithmetic on
// samples lives here: each unit has its own.
#pragma once
#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

#include "nc_common.h"

namespace nc {

constexpr int64_t kResampleMaxLen = (int64_t)1 << 30;        // samples per row
constexpr int64_t kResampleMaxTable = (int64_t)4 << 20;      // bytes of h[U][K4]: the L2 of one XCD
constexpr int64_t kResampleMaxOut = ((int64_t)1 << 31) - 256;   // outputs of one row that one launch covers (grid x block below 2^32)

struct ResampleGeom {
    int64_t U, D, W, K, K4;
    int zeros;
    double rolloff;
};

struct ResampleCfg {
    int zeros;
    double rolloff;
};

inline int64_t resample_gcd(int64_t a, int64_t b) {
    while (b) {
        const int64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

inline void resample_check_rates(int src, int dst) {
    if (src < 1 || dst < 1) fail(NC_EINVAL, "sample rates %d -> %d: both must be at least 1", src, dst);
}

// the checked config: NULL and zero fields are julius' defaults (the binary64 0.945, as julius has it); a given rolloff is widened
inline ResampleCfg resample_resolve_cfg(const nc_resample_cfg* cfg) {
    ResampleCfg c = {24, 0.945};
    if (cfg) {
        if (cfg->zeros != 0) c.zeros = cfg->zeros;
        if (cfg->rolloff != 0.0f) c.rolloff = (double)cfg->rolloff;
    }
    if (c.zeros < 1 || c.zeros > 64) fail(NC_EINVAL, "zeros = %d is not in [1, 64]", c.zeros);
    if (!(c.rolloff >= 0.5 && c.rolloff <= 1.0)) fail(NC_EINVAL, "rolloff = %g is not in [0.5, 1]", c.rolloff);
    return c;
}

// n_out = ceil(n U / D); n <= 2^30 and U < 2^31, so the product is exact
inline int64_t resample_len(int64_t n, int64_t U, int64_t D) { return (n * U + D - 1) / D; }

// NC_EINVAL unless the rates, the config and the table size are admitted
inline ResampleGeom resample_geom(int src, int dst, const nc_resample_cfg* cfg) {
    resample_check_rates(src, dst);
    const ResampleCfg c = resample_resolve_cfg(cfg);
    const int64_t g = resample_gcd(src, dst);
    ResampleGeom q;
    q.U = dst / g;
    q.D = src / g;
    q.zeros = c.zeros;
    q.rolloff = c.rolloff;
    const double base = (double)std::min(q.U, q.D) * c.rolloff;
    const double w = std::ceil((double)c.zeros * (double)q.D / base);
    // K4 <= 2^20 wherever the table is admitted: refuse before anything is narrowed
    if (!(w < 1048576.0)) fail(NC_EINVAL, "%d -> %d Hz: the filter table is above 4 MiB", src, dst);
    q.W = (int64_t)w;
    q.K = 2 * q.W + q.D;
    q.K4 = (q.K + 3) & ~(int64_t)3;
    if (q.U * q.K4 * 4 > kResampleMaxTable)
        fail(NC_EINVAL, "%d -> %d Hz: the filter table of %lld x %lld taps is above 4 MiB", src, dst, (long long)q.U, (long long)q.K4);
    return q;
}

// h[U][K4]: binary64, row by row divided by its own sum, rounded once
inline void build_resample_table(const ResampleGeom& q, std::vector<float>& h) {
    const double pi = 0x1.921fb54442d18p+1;
    const double base = (double)std::min(q.U, q.D) * q.rolloff, z = (double)q.zeros;
    h.assign((size_t)(q.U * q.K4), 0.0f);
    std::vector<double> v((size_t)q.K);
    for (int64_t i = 0; i < q.U; ++i) {
        double sum = 0.0;
        for (int64_t k = 0; k < q.K; ++k) {
            double t = ((-(double)i) / (double)q.U + (double)(k - q.W) / (double)q.D) * base;
            t = t < -z ? -z : (t > z ? z : t);
            const double a = pi * t;
            const double c = std::cos(a / (2.0 * z));
            v[(size_t)k] = (a == 0.0 ? 1.0 : std::sin(a) / a) * c * c;
            sum = sum + v[(size_t)k];
        }
        for (int64_t k = 0; k < q.K; ++k) h[(size_t)(i * q.K4 + k)] = (float)(v[(size_t)k] / sum);
    }
}

// the union of byte ranges as sorted disjoint intervals
inline void resample_merge(std::vector<std::pair<uintptr_t, uintptr_t>>& v) {
    std::sort(v.begin(), v.end());
    size_t w = 0;
    for (size_t i = 0; i < v.size(); ++i) {
        if (w > 0 && v[i].first <= v[w - 1].second)
            v[w - 1].second = std::max(v[w - 1].second, v[i].second);
        else
            v[w++] = v[i];
    }
    v.resize(w);
}

// the rows of a call: pointers, R in [1, 32767], offsets >= 0, 0 <= n <= 2^30, n_out within one launch, no output row over an input row
inline void resample_check_rows(const float* pcm, int R, const int64_t* off, const int64_t* n, const ResampleGeom& q, bool copy, const float* out,
                                const int64_t* out_off) {
    if (!pcm || !out || !off || !n || !out_off) fail(NC_EINVAL, "null pointer");
    if (R < 1 || R > 32767) fail(NC_EINVAL, "%d rows: not in [1, 32767]", R);
    std::vector<std::pair<uintptr_t, uintptr_t>> in, ou;
    for (int r = 0; r < R; ++r) {
        if (off[r] < 0 || out_off[r] < 0) fail(NC_EINVAL, "row %d has a negative offset", r);
        if (n[r] < 0) fail(NC_EINVAL, "row %d has a negative length", r);
        if (n[r] > kResampleMaxLen) fail(NC_EINVAL, "row %d is longer than 2^30 samples", r);
        const int64_t no = copy ? n[r] : resample_len(n[r], q.U, q.D);
        if (no > kResampleMaxOut) fail(NC_EINVAL, "row %d is too long for one launch", r);
        if (n[r] == 0) continue;
        const uintptr_t a = reinterpret_cast<uintptr_t>(pcm + off[r]), b = reinterpret_cast<uintptr_t>(out + out_off[r]);
        in.emplace_back(a, a + (uintptr_t)n[r] * sizeof(float));
        ou.emplace_back(b, b + (uintptr_t)no * sizeof(float));
    }
    resample_merge(in);
    resample_merge(ou);
    for (size_t i = 0, j = 0; i < in.size() && j < ou.size();) {
        if (in[i].first < ou[j].second && ou[j].first < in[i].second) fail(NC_EINVAL, "an output row overlaps an input row: the call never runs in place");
        if (in[i].second <= ou[j].second) ++i; else ++j;
    }
}

}  // namespace nc
