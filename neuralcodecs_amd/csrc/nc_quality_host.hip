// Round-trip quality as plain serial C++ on host memory (include/nc_mi355x.h "round-trip quality"): nc_audio_stft_host,
// nc_audio_mel_spectrogram_host, nc_quality_metrics_host, the two host table builders and the argument checks.  A product call (a CPU
// caller; a caller checking a device result) and the bit judge of the kernels in nc_quality.hip: written apart from them as loops over
// rows, frames and samples, sharing nc_math.h (nc_log10f), the tables and the checks below, and nothing else.  Built with
// -ffp-contract=off like every unit: each +, -, *, / is one rounding of its operand type, the same on the host as on gfx950.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <limits>
#include <vector>

#include "nc_guard.h"
#include "nc_math.h"
#include "nc_quality.h"

namespace nc {

void quality_check_window(int W, int H, int window) {
    if (W < 32 || W > 2048 || (W & (W - 1)) != 0) fail(NC_EINVAL, "window length %d is not a power of two in 32..2048", W);
    if (H < 1 || H > W || H > 512) fail(NC_EINVAL, "hop %d is not in [1, min(window = %d, 512)]", H, W);
    if (window != NC_WINDOW_HANN && window != NC_WINDOW_ONES) fail(NC_EINVAL, "unknown window type %d", window);
}

void quality_check_rows(int B, const int64_t* const* offs, int n_offs, const int64_t* n, const int* Ws, int n_W) {
    if (B < 1 || B > 32767) fail(NC_EINVAL, "B = %d is not in [1, 32767]", B);
    if (!n) fail(NC_EINVAL, "null pointer");
    for (int a = 0; a < n_offs; ++a)
        if (!offs[a]) fail(NC_EINVAL, "null pointer");
    for (int b = 0; b < B; ++b) {
        for (int a = 0; a < n_offs; ++a)
            if (offs[a][b] < 0) fail(NC_EINVAL, "row %d has a negative offset", b);
        if (n[b] > (int64_t)1 << 40) fail(NC_EINVAL, "row %d is too long", b);
        for (int i = 0; i < n_W; ++i)
            if (n[b] <= Ws[i] / 2) fail(NC_EINVAL, "row %d has %lld samples: reflect padding of window %d needs more than %d", b, (long long)n[b], Ws[i], Ws[i] / 2);
    }
}

void quality_check_mel(int sample_rate, int n_mels, float fmin, float fmax) {
    if (sample_rate <= 0) fail(NC_EINVAL, "sample rate must be positive");
    if (n_mels < 1 || n_mels > 512) fail(NC_EINVAL, "n_mels = %d is not in [1, 512]", n_mels);
    if (!(fmin >= 0.0f) || !std::isfinite(fmin)) fail(NC_EINVAL, "fmin must be finite and not negative");
    if (!(fmax > fmin) || !std::isfinite(fmax)) fail(NC_EINVAL, "fmax must be finite and above fmin");
}

nc_quality_cfg quality_resolve_cfg(const nc_quality_cfg* cfg, int sample_rate) {
    if (!cfg) fail(NC_EINVAL, "null pointer");
    nc_quality_cfg c = *cfg;
    if (c.n_scales < 1 || c.n_scales > NC_QUALITY_MAX_SCALES) fail(NC_EINVAL, "n_scales = %d is not in [1, %d]", c.n_scales, NC_QUALITY_MAX_SCALES);
    if (sample_rate <= 0) fail(NC_EINVAL, "sample rate must be positive");
    for (int i = 0; i < c.n_scales; ++i) {
        if (c.H[i] == 0) c.H[i] = c.W[i] / 4;
        if (c.fmax[i] == 0.0f) c.fmax[i] = (float)sample_rate / 2.0f;
        quality_check_window(c.W[i], c.H[i], NC_WINDOW_HANN);
        quality_check_mel(sample_rate, c.n_mels[i], c.fmin[i], c.fmax[i]);
    }
    if (!(c.clamp_eps >= 1e-18f) || !std::isfinite(c.clamp_eps)) fail(NC_EINVAL, "clamp_eps must be finite and at least 1e-18");
    if (!std::isfinite(c.log_weight) || !std::isfinite(c.mag_weight)) fail(NC_EINVAL, "the weights must be finite");
    return c;
}

void build_dft_basis(int W, int window, float* C, float* S) {
    const double two_pi = 2.0 * 3.14159265358979323846;
    std::vector<double> w((size_t)W);
    for (int n = 0; n < W; ++n) w[(size_t)n] = window == NC_WINDOW_ONES ? 1.0 : 0.5 - 0.5 * std::cos(two_pi * (double)n / (double)W);
    for (int k = 0; k <= W / 2; ++k)
        for (int n = 0; n < W; ++n) {
            const double ang = two_pi * (double)((k * n) % W) / (double)W;
            C[(size_t)k * W + n] = (float)(w[(size_t)n] * std::cos(ang));
            S[(size_t)k * W + n] = (float)(-w[(size_t)n] * std::sin(ang));
        }
}

void build_mel_filterbank(int sample_rate, int n_mels, int n_fft, float fmin, float fmax, float* fb, int32_t* lo, int32_t* hi) {
    const int K = n_fft / 2 + 1;
    auto to_mel = [](double hz) { return 2595.0 * std::log10(1.0 + hz / 700.0); };
    const double m0 = to_mel((double)fmin), m1 = to_mel((double)fmax);
    std::vector<double> hz((size_t)n_mels + 2);
    for (int i = 0; i < n_mels + 2; ++i) {
        const double mel = m0 + (m1 - m0) * (double)i / (double)(n_mels + 1);
        hz[(size_t)i] = 700.0 * (std::pow(10.0, mel / 2595.0) - 1.0);
    }
    for (int i = 0; i < n_mels; ++i) {
        const double left = hz[(size_t)i], center = hz[(size_t)i + 1], right = hz[(size_t)i + 2];
        const double enorm = 2.0 / (right - left);
        int first = -1, last = -1;
        for (int j = 0; j < K; ++j) {
            const double freq = (double)((int64_t)j * sample_rate) / (double)(2 * (K - 1));
            double v = 0.0;
            if (freq >= left && freq < center) v = (freq - left) / (center - left);
            else if (freq >= center && freq < right) v = (right - freq) / (right - center);
            if (freq >= left && freq < right) {
                if (first < 0) first = j;
                last = j;
            }
            fb[(size_t)i * K + j] = (float)(v * enorm);
        }
        if (lo) lo[i] = first < 0 ? 0 : first;
        if (hi) hi[i] = first < 0 ? 0 : last + 1;
    }
}

namespace {

// the reflect-padded row: W/2 samples mirrored about the first and the last sample
std::vector<float> padded_row(const float* x, int64_t n, int W) {
    const int half = W / 2;
    std::vector<float> p((size_t)(n + W));
    for (int64_t s = 0; s < n + W; ++s) {
        int64_t i = s - half;
        if (i < 0) i = -i;
        if (i >= n) i = 2 * (n - 1) - i;
        p[(size_t)s] = x[i];
    }
    return p;
}

// re / im [K][F] (nullable together) and mag [K][F] (nullable) of one row
void stft_row(const float* x, int64_t n, int W, int H, const float* C, const float* S, float* cplx, float* mag) {
    const int K = W / 2 + 1;
    const int64_t F = 1 + n / H;
    const std::vector<float> p = padded_row(x, n, W);
    for (int k = 0; k < K; ++k)
        for (int64_t t = 0; t < F; ++t) {
            float re = 0.0f, im = 0.0f;
            const float* xf = p.data() + t * H;
            for (int j = 0; j < W; ++j) {
                re = nc_fma(C[(size_t)k * W + j], xf[j], re);
                im = nc_fma(S[(size_t)k * W + j], xf[j], im);
            }
            if (cplx) {
                cplx[2 * ((int64_t)k * F + t)] = re;
                cplx[2 * ((int64_t)k * F + t) + 1] = im;
            }
            if (mag) {
                const float a = re * re, b = im * im;
                mag[(int64_t)k * F + t] = sqrtf(a + b);
            }
        }
}

struct MelTable {
    int K = 0, M = 0;
    std::vector<float> fb;
    std::vector<int32_t> lo, hi;
    MelTable(int sr, int n_mels, int W, float fmin, float fmax) : K(W / 2 + 1), M(n_mels), fb((size_t)n_mels * (W / 2 + 1)), lo((size_t)n_mels), hi((size_t)n_mels) {
        build_mel_filterbank(sr, n_mels, W, fmin, fmax, fb.data(), lo.data(), hi.data());
    }
};

void mel_row(const float* mag, int64_t F, const MelTable& mt, float* mel) {
    for (int m = 0; m < mt.M; ++m)
        for (int64_t t = 0; t < F; ++t) {
            float acc = 0.0f;
            for (int k = mt.lo[(size_t)m]; k < mt.hi[(size_t)m]; ++k) acc = nc_fma(mt.fb[(size_t)m * mt.K + k], mag[(int64_t)k * F + t], acc);
            mel[(int64_t)m * F + t] = acc;
        }
}

std::vector<float> mel_of_row(const float* x, int64_t n, int W, int H, const float* C, const float* S, const MelTable& mt) {
    const int64_t F = 1 + n / H;
    std::vector<float> mag((size_t)((int64_t)(W / 2 + 1) * F)), mel((size_t)((int64_t)mt.M * F));
    stft_row(x, n, W, H, C, S, nullptr, mag.data());
    mel_row(mag.data(), F, mt, mel.data());
    return mel;
}

float log_mel(float v, float clamp_eps) {
    const float c = v > clamp_eps ? v : clamp_eps;   // a NaN takes the clamp; rows with NaN samples never get here
    return nc_log10f(c * c);
}

struct Basis {
    std::vector<float> C, S;
    Basis(int W, int window) : C((size_t)(W / 2 + 1) * W), S((size_t)(W / 2 + 1) * W) { build_dft_basis(W, window, C.data(), S.data()); }
};

}  // namespace

}  // namespace nc

using namespace nc;

extern "C" int64_t nc_audio_stft_frames(int64_t n, int32_t W, int32_t H) {
    if (W < 2 || H < 1 || n <= W / 2) return -1;
    return 1 + n / H;
}

extern "C" nc_status nc_op_log10f(const float* x, int64_t n, float* y) {
    return guard([&] {
        if (!x || !y || n < 0) fail(NC_EINVAL, "null pointer or negative count");
        for (int64_t i = 0; i < n; ++i) y[i] = nc_log10f(x[i]);
    });
}

extern "C" nc_status nc_audio_dft_basis(int32_t W, int32_t window, float* C, float* S) {
    return guard([&] {
        if (!C || !S) fail(NC_EINVAL, "null pointer");
        quality_check_window(W, 1, window);
        build_dft_basis(W, window, C, S);
    });
}

extern "C" nc_status nc_audio_mel_filterbank(int32_t sample_rate, int32_t n_mels, int32_t n_fft, float fmin, float fmax, float* fb, int32_t* lo,
                                             int32_t* hi) {
    return guard([&] {
        if (!fb) fail(NC_EINVAL, "null pointer");
        if (n_fft < 2 || n_fft > 1 << 16 || (n_fft & 1)) fail(NC_EINVAL, "n_fft = %d is not an even number in 2..65536", n_fft);
        if (fmax == 0.0f && sample_rate > 0) fmax = (float)sample_rate / 2.0f;
        quality_check_mel(sample_rate, n_mels, fmin, fmax);
        build_mel_filterbank(sample_rate, n_mels, n_fft, fmin, fmax, fb, lo, hi);
    });
}

extern "C" nc_status nc_audio_stft_host(const float* pcm, int32_t B, const int64_t* off, const int64_t* n, int32_t W, int32_t H, int32_t window,
                                        float* out_c64, const int64_t* out_off) {
    return guard([&] {
        if (!pcm || !out_c64) fail(NC_EINVAL, "null pointer");
        quality_check_window(W, H, window);
        const int64_t* offs[2] = {off, out_off};
        quality_check_rows(B, offs, 2, n, &W, 1);
        const Basis bs(W, window);
        for (int b = 0; b < B; ++b) stft_row(pcm + off[b], n[b], W, H, bs.C.data(), bs.S.data(), out_c64 + 2 * out_off[b], nullptr);
    });
}

extern "C" nc_status nc_audio_mel_spectrogram_host(const float* pcm, int32_t B, const int64_t* off, const int64_t* n, int32_t sample_rate, int32_t W,
                                                   int32_t H, int32_t n_mels, float fmin, float fmax, float* out, const int64_t* out_off) {
    return guard([&] {
        if (!pcm || !out) fail(NC_EINVAL, "null pointer");
        quality_check_window(W, H, NC_WINDOW_HANN);
        if (fmax == 0.0f && sample_rate > 0) fmax = (float)sample_rate / 2.0f;
        quality_check_mel(sample_rate, n_mels, fmin, fmax);
        const int64_t* offs[2] = {off, out_off};
        quality_check_rows(B, offs, 2, n, &W, 1);
        const Basis bs(W, NC_WINDOW_HANN);
        const MelTable mt(sample_rate, n_mels, W, fmin, fmax);
        for (int b = 0; b < B; ++b) {
            const std::vector<float> mel = mel_of_row(pcm + off[b], n[b], W, H, bs.C.data(), bs.S.data(), mt);
            std::copy(mel.begin(), mel.end(), out + out_off[b]);
        }
    });
}

extern "C" nc_status nc_quality_metrics_host(const float* ref, const int64_t* ref_off, const float* est, const int64_t* est_off, const int64_t* n,
                                             int32_t B, int32_t sample_rate, const nc_quality_cfg* cfg, nc_quality_row* out) {
    return guard([&] {
        if (!ref || !est || !out) fail(NC_EINVAL, "null pointer");
        const nc_quality_cfg c = quality_resolve_cfg(cfg, sample_rate);
        const int64_t* offs[2] = {ref_off, est_off};
        quality_check_rows(B, offs, 2, n, c.W, c.n_scales);
        const double EPS = (double)1e-8f;
        const float nan = std::numeric_limits<float>::quiet_NaN();
        std::vector<Basis> bases;
        std::vector<MelTable> mels;
        for (int i = 0; i < c.n_scales; ++i) {
            bases.emplace_back(c.W[i], NC_WINDOW_HANN);
            mels.emplace_back(sample_rate, c.n_mels[i], c.W[i], c.fmin[i], c.fmax[i]);
        }
        for (int b = 0; b < B; ++b) {
            const float* x = est + est_off[b];
            const float* y = ref + ref_off[b];
            const int64_t N = n[b], nblk = (N + kQualityBlock - 1) / kQualityBlock;
            nc_quality_row r = {};
            double Sx = 0.0, Sy = 0.0, Sl1 = 0.0;
            int64_t bad = 0;
            for (int64_t q = 0; q < nblk; ++q) {
                double sx = 0.0, sy = 0.0, sl = 0.0;
                for (int64_t i = q * kQualityBlock; i < N && i < (q + 1) * kQualityBlock; ++i) {
                    sx = sx + (double)x[i];
                    sy = sy + (double)y[i];
                    const float d = x[i] - y[i];
                    sl = sl + (double)__builtin_fabsf(d);
                    bad += (finite32(x[i]) ? 0 : 1) + (finite32(y[i]) ? 0 : 1);
                }
                Sx = Sx + sx;
                Sy = Sy + sy;
                Sl1 = Sl1 + sl;
            }
            r.n_bad = (int32_t)(bad > 0x7fffffff ? 0x7fffffff : bad);
            if (bad) {
                r.l1 = r.si_sdr_db = r.mel_distance = nan;
                for (int i = 0; i < c.n_scales; ++i) r.mel_log[i] = r.mel_mag[i] = nan;
                out[b] = r;
                continue;
            }
            const double mx = Sx / (double)N, my = Sy / (double)N;
            double Syy = 0.0, Sxy = 0.0;
            for (int64_t q = 0; q < nblk; ++q) {
                double syy = 0.0, sxy = 0.0;
                for (int64_t i = q * kQualityBlock; i < N && i < (q + 1) * kQualityBlock; ++i) {
                    const double xc = (double)x[i] - mx, yc = (double)y[i] - my;
                    syy = syy + yc * yc;
                    sxy = sxy + xc * yc;
                }
                Syy = Syy + syy;
                Sxy = Sxy + sxy;
            }
            const double scale = (Sxy + EPS) / (Syy + EPS);
            double See = 0.0;
            for (int64_t q = 0; q < nblk; ++q) {
                double see = 0.0;
                for (int64_t i = q * kQualityBlock; i < N && i < (q + 1) * kQualityBlock; ++i) {
                    const double xc = (double)x[i] - mx, yc = (double)y[i] - my;
                    const double e = xc - scale * yc;
                    see = see + e * e;
                }
                See = See + see;
            }
            const double target = scale * scale * Syy;
            double ratio = target / (See + EPS) + EPS;
            if (ratio > (double)FLT_MAX) ratio = (double)FLT_MAX;
            r.l1 = (float)(Sl1 / (double)N);
            r.si_sdr_db = 10.0f * nc_log10f((float)ratio);
            double dist = 0.0;
            for (int i = 0; i < c.n_scales; ++i) {
                const Basis& bs = bases[(size_t)i];
                const MelTable& mt = mels[(size_t)i];
                const std::vector<float> X = mel_of_row(x, N, c.W[i], c.H[i], bs.C.data(), bs.S.data(), mt);
                const std::vector<float> Y = mel_of_row(y, N, c.W[i], c.H[i], bs.C.data(), bs.S.data(), mt);
                const int64_t F = 1 + N / c.H[i];
                double Smag = 0.0, Slog = 0.0;
                for (int64_t t = 0; t < F; ++t) {
                    double fm = 0.0, fl = 0.0;
                    for (int m = 0; m < mt.M; ++m) {
                        const float a = X[(size_t)((int64_t)m * F + t)], bq = Y[(size_t)((int64_t)m * F + t)];
                        const float d = a - bq;
                        fm = fm + (double)__builtin_fabsf(d);
                        const float dl = log_mel(a, c.clamp_eps) - log_mel(bq, c.clamp_eps);
                        fl = fl + (double)__builtin_fabsf(dl);
                    }
                    Smag = Smag + fm;
                    Slog = Slog + fl;
                }
                const double cnt = (double)((int64_t)mt.M * F);
                const double mean_mag = Smag / cnt, mean_log = Slog / cnt;
                r.mel_mag[i] = (float)mean_mag;
                r.mel_log[i] = (float)mean_log;
                dist = dist + ((double)c.log_weight * mean_log + (double)c.mag_weight * mean_mag);
            }
            r.mel_distance = (float)dist;
            out[b] = r;
        }
    });
}
