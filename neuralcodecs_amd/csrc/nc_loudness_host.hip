// Loudness as plain serial C++ on host memory (include/nc_mi355x.h "loudness"): nc_audio_kweight_host, nc_loudness_host,
// nc_loudness_normalize_host, nc_audio_apply_gain_db_host, the coefficient source, the block-table builder and the argument checks.  A
// product call (a CPU caller; a caller checking a device result) and the bit judge of the kernels in nc_loudness.hip: written apart from
// them as loops over clips, channels, blocks and samples, sharing nc_math.h (nc_fma, nc_log10f, nc_expf), the tables and the checks below,
// and nothing else.  Built with -ffp-contract=off like every unit: each +, -, *, / is one rounding of its operand type, the same on the
// host as on gfx950.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <limits>
#include <vector>

#include "nc_guard.h"
#include "nc_loudness.h"
#include "nc_math.h"

namespace nc {

void loudness_check_filter(int sample_rate, int filter) {
    if (sample_rate < 10) fail(NC_EINVAL, "sample rate %d is below 10: the gating block or its step would be empty", sample_rate);
    if (filter != NC_KWEIGHT_REFERENCE && filter != NC_KWEIGHT_DESIGNED) fail(NC_EINVAL, "unknown K-weighting filter %d", filter);
}

void loudness_check_rows(int R, const int64_t* const* offs, int n_offs, int rows_per_n, const int64_t* n) {
    if (R < 1 || R > 32767) fail(NC_EINVAL, "%d rows: not in [1, 32767]", R);
    if (!n) fail(NC_EINVAL, "null pointer");
    for (int a = 0; a < n_offs; ++a)
        if (!offs[a]) fail(NC_EINVAL, "null pointer");
    for (int r = 0; r < R; ++r) {
        for (int a = 0; a < n_offs; ++a)
            if (offs[a][r] < 0) fail(NC_EINVAL, "row %d has a negative offset", r);
        const int64_t len = n[r / rows_per_n];
        if (len < 0) fail(NC_EINVAL, "row %d has a negative length", r);
        if (len > (int64_t)1 << 36) fail(NC_EINVAL, "row %d is too long", r);
    }
}

void loudness_check_clips(int B, int C, const int64_t* const* offs, int n_offs, const int64_t* n) {
    if (B < 1) fail(NC_EINVAL, "B = %d is not positive", B);
    if (C < 1 || C > NC_LOUDNESS_MAX_CHANNELS) fail(NC_EINVAL, "C = %d is not in [1, %d]", C, NC_LOUDNESS_MAX_CHANNELS);
    if ((int64_t)B * C > 32767) fail(NC_EINVAL, "B C = %lld is above 32767", (long long)B * C);
    loudness_check_rows(B * C, offs, n_offs, C, n);
}

nc_loudness_cfg loudness_resolve_cfg(const nc_loudness_cfg* cfg, int sample_rate) {
    if (!cfg) fail(NC_EINVAL, "null pointer");
    loudness_check_filter(sample_rate, cfg->filter);
    if (!std::isfinite(cfg->target_db)) fail(NC_EINVAL, "the target level must be finite");
    return *cfg;
}

LoudGeom loudness_geom(int sample_rate) {
    const float block = 0.4f * (float)sample_rate;
    const float step = block * 0.25f;
    return LoudGeom{(int)block, (int)step};
}

void kweight_coeffs(int sample_rate, int filter, double* b, double* a) {
    if (filter == NC_KWEIGHT_REFERENCE) {
        const float rb[2][3] = {{1.53512485958697f, -2.69169618940638f, 1.19839281085285f}, {1.0f, -2.0f, 1.0f}};
        const float ra[2][3] = {{1.0f, -1.69065929318241f, 0.73248077421585f}, {1.0f, -1.99004745483398f, 0.99007225036621f}};
        for (int s = 0; s < 2; ++s)
            for (int i = 0; i < 3; ++i) {
                b[3 * s + i] = (double)rb[s][i];
                a[3 * s + i] = (double)ra[s][i];
            }
        return;
    }
    // The analog prototypes behind the BS.1770 constants (De Man, "Evaluation of implementations of the EBU R128 loudness measurement",
    // AES 145, 2018), through the bilinear transform with K = tan(pi f0 / rate): at 48 kHz they give the constants back.
    const double pi = 3.14159265358979323846, fs = (double)sample_rate;
    {   // high shelf: 1681.97 Hz, +3.9998 dB, Q = 0.70718
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(pi * f0 / fs), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        b[0] = (Vh + Vb * K / Q + K * K) / a0;
        b[1] = 2.0 * (K * K - Vh) / a0;
        b[2] = (Vh - Vb * K / Q + K * K) / a0;
        a[0] = 1.0;
        a[1] = 2.0 * (K * K - 1.0) / a0;
        a[2] = (1.0 - K / Q + K * K) / a0;
    }
    {   // high pass: 38.135 Hz, Q = 0.50033; the numerator stays (1, -2, 1) as in the recommendation
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(pi * f0 / fs), a0 = 1.0 + K / Q + K * K;
        b[3] = 1.0;
        b[4] = -2.0;
        b[5] = 1.0;
        a[3] = 1.0;
        a[4] = 2.0 * (K * K - 1.0) / a0;
        a[5] = (1.0 - K / Q + K * K) / a0;
    }
}

void build_kweight_tables(int sample_rate, int filter, KwTables& t) {
    constexpr int L = kKwBlock;
    double b[6], a[6];
    kweight_coeffs(sample_rate, filter, b, a);
    const double b0 = b[0], b1 = b[1], b2 = b[2], a1 = a[1], a2 = a[2];
    const double c0 = b[3], c1 = b[4], c2 = b[5], d1 = a[4], d2 = a[5];
    const double e1 = c1 - d1 * c0, e2 = c2 - d2 * c0;
    const double A[4][4] = {{-a1, 1.0, 0.0, 0.0}, {-a2, 0.0, 0.0, 0.0}, {e1, 0.0, -d1, 1.0}, {e2, 0.0, -d2, 0.0}};
    const double Bv[4] = {b1 - a1 * b0, b2 - a2 * b0, e1 * b0, e2 * b0};
    const double Cv[4] = {c0, 0.0, 1.0, 0.0};
    const double D = c0 * b0;
    auto dot4 = [](const double* p, const double* q, int qs) {   // ascending from the first product
        double acc = p[0] * q[0];
        for (int k = 1; k < 4; ++k) acc = acc + p[k] * q[(size_t)k * qs];
        return acc;
    };
    // AkB[k] = A^k B, k = 0..L-1
    std::vector<double> AkB((size_t)L * 4);
    for (int i = 0; i < 4; ++i) AkB[(size_t)i] = Bv[i];
    for (int k = 1; k < L; ++k)
        for (int i = 0; i < 4; ++i) AkB[(size_t)k * 4 + i] = dot4(A[i], &AkB[(size_t)(k - 1) * 4], 1);
    double h[L];
    h[0] = D;
    for (int k = 1; k < L; ++k) h[k] = dot4(Cv, &AkB[(size_t)(k - 1) * 4], 1);
    t.Hm.assign((size_t)L * L, 0.0f);
    t.Cm.assign((size_t)4 * L, 0.0f);
    for (int r = 0; r < L; ++r)
        for (int j = 0; j <= r; ++j) t.Hm[(size_t)r * L + j] = (float)h[r - j];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < L; ++j) t.Cm[(size_t)i * L + j] = (float)AkB[(size_t)(L - 1 - j) * 4 + i];
    // Gs[r] = C A^r
    for (int i = 0; i < 4; ++i) t.Gs[0][i] = Cv[i];
    for (int r = 1; r < L; ++r)
        for (int i = 0; i < 4; ++i) t.Gs[r][i] = dot4(t.Gs[r - 1], &A[0][i], 4);
    // M = A^L by left multiplication
    double P[4][4], Q[4][4];
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 4; ++k) P[i][k] = A[i][k];
    for (int p = 1; p < L; ++p) {
        for (int i = 0; i < 4; ++i)
            for (int k = 0; k < 4; ++k) Q[i][k] = dot4(A[i], &P[0][k], 4);
        for (int i = 0; i < 4; ++i)
            for (int k = 0; k < 4; ++k) P[i][k] = Q[i][k];
    }
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 4; ++k) t.M[i][k] = P[i][k];
}

namespace {

double dot_state(const double* w, const double* s) { return ((w[0] * s[0] + w[1] * s[1]) + w[2] * s[2]) + w[3] * s[3]; }

// y[0..n) of one row, block by block
void kweight_row(const KwTables& t, const float* x, int64_t n, float* y) {
    constexpr int L = kKwBlock;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t q0 = 0; q0 < n; q0 += L) {
        float xb[L];
        for (int j = 0; j < L; ++j) xb[j] = q0 + j < n ? x[q0 + j] : 0.0f;
        for (int r = 0; r < L && q0 + r < n; ++r) {
            float u = 0.0f;
            for (int j = 0; j < L; ++j) u = nc_fma(t.Hm[(size_t)r * L + j], xb[j], u);
            y[q0 + r] = (float)((double)u + dot_state(t.Gs[r], s));
        }
        double s1[4];
        for (int i = 0; i < 4; ++i) {
            float v = 0.0f;
            for (int j = 0; j < L; ++j) v = nc_fma(t.Cm[(size_t)i * L + j], xb[j], v);
            s1[i] = dot_state(t.M[i], s) + (double)v;
        }
        for (int i = 0; i < 4; ++i) s[i] = s1[i];
    }
}

// z[j], j = 0..J-1, of one filtered row
void block_energies(const float* y, int64_t J, const LoudGeom& g, double* z) {
    if (J <= 0) return;
    const int64_t S = g.S, N = g.N, ncell = J + 3;
    std::vector<double> cell((size_t)ncell);
    for (int64_t i = 0; i < ncell; ++i) {
        double acc = 0.0;
        for (int64_t k0 = 0; k0 < S; k0 += kLoudSub) {
            double sub = 0.0;
            for (int64_t k = k0; k < S && k < k0 + kLoudSub; ++k) {
                const float v = y[i * S + k];
                sub = sub + (double)(v * v);
            }
            acc = acc + sub;
        }
        cell[(size_t)i] = acc;
    }
    for (int64_t j = 0; j < J; ++j) {
        double sum = ((cell[(size_t)j] + cell[(size_t)j + 1]) + cell[(size_t)j + 2]) + cell[(size_t)j + 3];
        for (int64_t k = (j + 4) * S; k < j * S + N; ++k) {
            const float v = y[k];
            sum = sum + (double)(v * v);
        }
        z[j] = sum / (double)N;
    }
}

const float kChannelGain[NC_LOUDNESS_MAX_CHANNELS] = {1.0f, 1.0f, 1.0f, 1.41f, 1.41f};

nc_loudness_row measure_clip(const KwTables& t, const LoudGeom& g, const float* pcm, const int64_t* off, int C, int64_t n, float target_db) {
    nc_loudness_row r = {};
    const int64_t J = n >= g.N ? (n - g.N) / g.S + 1 : 0;
    r.n_blocks = (int32_t)(J > 0x7fffffff ? 0x7fffffff : J);
    int64_t bad = 0;
    for (int c = 0; c < C; ++c)
        for (int64_t i = 0; i < n; ++i) bad += finite32(pcm[off[c] + i]) ? 0 : 1;
    r.n_bad = (int32_t)(bad > 0x7fffffff ? 0x7fffffff : bad);
    if (bad) {
        r.lufs = r.gain = std::numeric_limits<float>::quiet_NaN();
        return r;
    }
    std::vector<float> y((size_t)n);
    std::vector<double> z((size_t)C * (size_t)J), W((size_t)J);
    for (int c = 0; c < C; ++c) {
        kweight_row(t, pcm + off[c], n, y.data());
        block_energies(y.data(), J, g, z.data() + (size_t)c * (size_t)J);
    }
    for (int64_t j = 0; j < J; ++j) {
        double w = 0.0;
        for (int c = 0; c < C; ++c) w = w + (double)kChannelGain[c] * z[(size_t)c * (size_t)J + (size_t)j];
        W[(size_t)j] = w;
    }
    int64_t na = 0, nr = 0;
    double Wa = 0.0, Wr = 0.0;
    for (int64_t j = 0; j < J; ++j) na += W[(size_t)j] > kGateAbs ? 1 : 0;
    for (int c = 0; c < C; ++c) {
        double acc = 0.0;
        for (int64_t j = 0; j < J; ++j)
            if (W[(size_t)j] > kGateAbs) acc = acc + z[(size_t)c * (size_t)J + (size_t)j];
        Wa = Wa + (double)kChannelGain[c] * (acc / (double)(na > 1 ? na : 1));
    }
    const double rel = 0.1 * Wa;
    for (int64_t j = 0; j < J; ++j) nr += (W[(size_t)j] > kGateAbs && W[(size_t)j] > rel) ? 1 : 0;
    for (int c = 0; c < C; ++c) {
        double acc = 0.0;
        for (int64_t j = 0; j < J; ++j)
            if (W[(size_t)j] > kGateAbs && W[(size_t)j] > rel) acc = acc + z[(size_t)c * (size_t)J + (size_t)j];
        Wr = Wr + (double)kChannelGain[c] * (acc / (double)(nr > 1 ? nr : 1));
    }
    r.n_pass_abs = (int32_t)(na > 0x7fffffff ? 0x7fffffff : na);
    r.n_pass_rel = (int32_t)(nr > 0x7fffffff ? 0x7fffffff : nr);
    const float wf = (float)Wr;
    float lufs = -70.0f;
    if (wf >= FLT_MIN) {
        const float l = -0.691f + 10.0f * nc_log10f(wf);
        lufs = l > -70.0f ? l : -70.0f;
    }
    r.lufs = lufs;
    r.gain = nc_expf((target_db - lufs) * kGainFactor);
    return r;
}

void scale_row(const float* x, int64_t n, float gain, float* out) {
    if (gain != gain) {
        const float qnan = __builtin_bit_cast(float, 0x7fc00000u);
        for (int64_t i = 0; i < n; ++i) out[i] = qnan;
        return;
    }
    for (int64_t i = 0; i < n; ++i) out[i] = x[i] * gain;
}

}  // namespace

}  // namespace nc

using namespace nc;

extern "C" nc_status nc_audio_kweight_coeffs(int32_t sample_rate, int32_t filter, double* b, double* a) {
    return guard([&] {
        if (!b || !a) fail(NC_EINVAL, "null pointer");
        loudness_check_filter(sample_rate, filter);
        kweight_coeffs(sample_rate, filter, b, a);
    });
}

extern "C" nc_status nc_audio_kweight_tables(int32_t sample_rate, int32_t filter, float* Hm, float* Cm, double* Gs, double* M) {
    return guard([&] {
        if (!Hm || !Cm || !Gs || !M) fail(NC_EINVAL, "null pointer");
        loudness_check_filter(sample_rate, filter);
        KwTables t;
        build_kweight_tables(sample_rate, filter, t);
        std::copy(t.Hm.begin(), t.Hm.end(), Hm);
        std::copy(t.Cm.begin(), t.Cm.end(), Cm);
        for (int r = 0; r < kKwBlock; ++r)
            for (int i = 0; i < 4; ++i) Gs[4 * r + i] = t.Gs[r][i];
        for (int i = 0; i < 4; ++i)
            for (int k = 0; k < 4; ++k) M[4 * i + k] = t.M[i][k];
    });
}

extern "C" nc_status nc_audio_kweight_host(const float* pcm, int32_t R, const int64_t* off, const int64_t* n, int32_t sample_rate, int32_t filter,
                                           float* out, const int64_t* out_off) {
    return guard([&] {
        if (!pcm || !out) fail(NC_EINVAL, "null pointer");
        loudness_check_filter(sample_rate, filter);
        const int64_t* offs[2] = {off, out_off};
        loudness_check_rows(R, offs, 2, 1, n);
        KwTables t;
        build_kweight_tables(sample_rate, filter, t);
        for (int r = 0; r < R; ++r) kweight_row(t, pcm + off[r], n[r], out + out_off[r]);
    });
}

extern "C" nc_status nc_loudness_host(const float* pcm, int32_t B, int32_t C, const int64_t* off, const int64_t* n, int32_t sample_rate,
                                      const nc_loudness_cfg* cfg, nc_loudness_row* out) {
    return guard([&] {
        if (!pcm || !out) fail(NC_EINVAL, "null pointer");
        const nc_loudness_cfg c = loudness_resolve_cfg(cfg, sample_rate);
        const int64_t* offs[1] = {off};
        loudness_check_clips(B, C, offs, 1, n);
        KwTables t;
        build_kweight_tables(sample_rate, c.filter, t);
        const LoudGeom g = loudness_geom(sample_rate);
        for (int b = 0; b < B; ++b) out[b] = measure_clip(t, g, pcm, off + (size_t)b * C, C, n[b], c.target_db);
    });
}

extern "C" nc_status nc_loudness_normalize_host(const float* pcm, int32_t B, int32_t C, const int64_t* off, const int64_t* n, int32_t sample_rate,
                                                const nc_loudness_cfg* cfg, float* out, const int64_t* out_off, nc_loudness_row* rows) {
    return guard([&] {
        if (!pcm || !out || !rows) fail(NC_EINVAL, "null pointer");
        const nc_loudness_cfg c = loudness_resolve_cfg(cfg, sample_rate);
        const int64_t* offs[2] = {off, out_off};
        loudness_check_clips(B, C, offs, 2, n);
        KwTables t;
        build_kweight_tables(sample_rate, c.filter, t);
        const LoudGeom g = loudness_geom(sample_rate);
        for (int b = 0; b < B; ++b) {
            rows[b] = measure_clip(t, g, pcm, off + (size_t)b * C, C, n[b], c.target_db);
            for (int ch = 0; ch < C; ++ch) scale_row(pcm + off[(size_t)b * C + ch], n[b], rows[b].gain, out + out_off[(size_t)b * C + ch]);
        }
    });
}

extern "C" nc_status nc_audio_apply_gain_db_host(const float* pcm, int32_t B, int32_t C, const int64_t* off, const int64_t* n, const float* db,
                                                 float* out, const int64_t* out_off) {
    return guard([&] {
        if (!pcm || !out || !db) fail(NC_EINVAL, "null pointer");
        const int64_t* offs[2] = {off, out_off};
        loudness_check_clips(B, C, offs, 2, n);
        for (int b = 0; b < B; ++b)
            if (!std::isfinite(db[b])) fail(NC_EINVAL, "db[%d] is not finite", b);
        for (int b = 0; b < B; ++b) {
            const float gain = nc_expf(db[b] * kGainFactor);
            for (int ch = 0; ch < C; ++ch) scale_row(pcm + off[(size_t)b * C + ch], n[b], gain, out + out_off[(size_t)b * C + ch]);
        }
    });
}
