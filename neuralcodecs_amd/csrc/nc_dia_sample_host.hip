// nc_dia_sample_host: Dia's sampling stage (include/nc_mi355x.h, "Dia sampling stage") as plain serial C++ on host memory.
// A product call (a CPU caller; a caller checking a device result) and the bit judge of the kernel in nc_dia.hip: written apart from it,
// row by row with std::stable_sort and loops, sharing nc_math.h (nc_expf) and nothing else.  The unit is built with -ffp-contract=off like
// every other: each +, -, *, / below is one binary32 rounding, the same on the host as on gfx950.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "nc_guard.h"
#include "nc_math.h"

namespace nc {

namespace {

// The limits of the header, named here as the kernel's side names its own (kDiaMaxC, kSampleMaxV, kSampleMaxK in nc_dia.hip): the two
// units share no code on purpose; tests/test_dia_sample_cpu.py holds both to the same refusals at the same values.
constexpr int kHostMaxC = 32, kHostMaxV = 4096, kHostMaxK = 64;

// the token of one row; -1 with *bad set where the definition gives none
int64_t sample_row_host(const float* uncond, const float* cond, int V, int c, const nc_dia_sample_params& p, float u, bool* bad) {
    const float ninf = -std::numeric_limits<float>::infinity();
    std::vector<float> g((size_t)V);
    for (int v = 0; v < V; ++v) {                                   // 1 guidance, 2 masks
        const float diff = cond[v] - uncond[v];
        const float scaled = p.cfg_scale * diff;
        g[(size_t)v] = cond[v] + scaled;
        if (v > p.eos) g[(size_t)v] = ninf;
        if (c >= 1 && v >= p.eos) g[(size_t)v] = ninf;
    }
    if (c == 0) g[(size_t)p.eos] = g[(size_t)p.eos] * 0.8f;
    int top = 0;                                                    // ATen's argmax: first maximum, a NaN beats every number, first NaN wins
    bool any_nan = std::isnan(g[0]);
    for (int v = 1; v < V; ++v) {
        const float x = g[(size_t)v], t = g[(size_t)top];
        if (std::isnan(x)) {
            any_nan = true;
            if (!std::isnan(t)) top = v;
        } else if (!std::isnan(t) && x > t) {
            top = v;
        }
    }
    *bad = false;
    if (p.temperature < 1e-5f) return top;                          // 3 greedy
    *bad = true;
    if (any_nan) return -1;                                         // 9
    if (top != p.eos) g[(size_t)p.eos] = ninf;                      // 4 EOS rule
    std::vector<int> order;
    for (int v = 0; v < V; ++v) {
        g[(size_t)v] = g[(size_t)v] / p.temperature;                // 5
        if (g[(size_t)v] > ninf) order.push_back(v);
    }
    // 6: value descending; stable over ascending indices, so equal values stay in index order
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return g[(size_t)a] > g[(size_t)b]; });
    if (order.size() > (size_t)p.top_k) order.resize((size_t)p.top_k);
    const size_t n = order.size();
    if (n == 0 || g[(size_t)order[0]] == std::numeric_limits<float>::infinity()) return -1;
    *bad = false;
    std::vector<float> e(n);
    for (size_t j = 0; j < n; ++j) e[j] = nc_expf(g[(size_t)order[j]] - g[(size_t)order[0]]);
    std::vector<char> kept(n, 1);
    if (p.top_p < 1.0f) {                                           // 7 nucleus
        float S = 0.0f;
        for (size_t j = 0; j < n; ++j) S = S + e[j];
        float cum = 0.0f;
        for (size_t j = 0; j < n; ++j) {
            if (j >= 1 && cum > p.top_p) kept[j] = 0;               // cum is c_{j-1} here
            const float pj = e[j] / S;
            cum = cum + pj;
        }
    }
    float S2 = 0.0f;                                                // 8 draw
    for (size_t j = 0; j < n; ++j)
        if (kept[j]) S2 = S2 + e[j];
    float d = 0.0f;
    size_t last = 0;
    for (size_t j = 0; j < n; ++j) {
        if (!kept[j]) continue;
        const float q = e[j] / S2;
        d = d + q;
        last = j;
        if (u < d) return order[j];
    }
    return order[last];
}

}  // namespace

}  // namespace nc

using namespace nc;

extern "C" nc_status nc_dia_sample_host(const float* logits, int32_t B, int32_t C, int32_t V, const nc_dia_sample_params* params, const float* uniform,
                                        int64_t* tokens, int32_t* bad) {
    return guard([&] {
        if (!logits || !params || !uniform || !tokens || !bad) fail(NC_EINVAL, "null pointer");
        const nc_dia_sample_params& p = *params;
        if (B <= 0) fail(NC_EINVAL, "B must be positive");
        if (C < 1 || C > kHostMaxC) fail(NC_EINVAL, "a row set has 1 to %d channels, not %d", kHostMaxC, C);
        if (V > kHostMaxV) fail(NC_EINVAL, "V = %d is above %d", V, kHostMaxV);
        if (p.eos < 0 || p.eos >= V) fail(NC_EINVAL, "eos = %d is not in [0, V = %d)", p.eos, V);
        if (p.top_k < 1 || p.top_k > kHostMaxK) fail(NC_EINVAL, "top_k = %d is not in [1, %d]", p.top_k, kHostMaxK);
        if (!std::isfinite(p.temperature) || !std::isfinite(p.top_p) || !std::isfinite(p.cfg_scale))
            fail(NC_EINVAL, "temperature, top_p and cfg_scale must be finite");
        if (p.temperature < 0.0f) fail(NC_EINVAL, "temperature must not be negative");
        if (p.top_p <= 0.0f) fail(NC_EINVAL, "top_p must be positive");
        for (int b = 0; b < B; ++b) {
            bad[b] = 0;
            for (int c = 0; c < C; ++c) {
                const float* uncond = logits + ((int64_t)(2 * b) * C + c) * V;
                bool row_bad = false;
                tokens[(int64_t)b * C + c] = sample_row_host(uncond, uncond + (int64_t)C * V, V, c, p, uniform[(int64_t)b * C + c], &row_bad);
                if (row_bad) bad[b] = 1;
            }
        }
    });
}
