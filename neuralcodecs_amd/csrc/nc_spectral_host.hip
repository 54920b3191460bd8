// Inverse STFT, spectral masks and MFCC as plain serial C++ on host memory (include/nc_mi355x.h "inverse STFT, spectral masks, MFCC",
// DESIGN.md 4q): the *_host calls, the table exports and the index helpers of the masks.  A product call (a CPU caller; a caller checking
// a device result) and the bit judge of the kernels in nc_spectral.hip: written apart from them as loops over rows, frames and samples,
// sharing nc_math.h (nc_fma, nc_logf), the tables and the checks of nc_spectral.h, and nothing else.  Built with -ffp-contract=off like
// every unit.
#include <algorithm>
#include <vector>

#include "nc_guard.h"
#include "nc_math.h"
#include "nc_spectral.h"

namespace nc {

namespace {

constexpr uint32_t kQuietNan = 0x7fc00000u;

// one row: the frames y[t][n], then every output sample from the frames that cover it
void istft_row(const float* spec, int64_t F, int W, int H, const float* T, const float* w32, float* out, int64_t L) {
    const int J = W + 2;
    std::vector<float> y((size_t)(F * W));
    for (int64_t t = 0; t < F; ++t)
        for (int n = 0; n < W; ++n) {
            float acc = 0.0f;
            for (int j = 0; j < J; ++j) acc = nc_fma(T[(size_t)n * J + j], spec[2 * ((int64_t)(j >> 1) * F + t) + (j & 1)], acc);
            y[(size_t)(t * W + n)] = acc;
        }
    const int64_t span = (int64_t)W + (int64_t)H * (F - 1);
    for (int64_t i = 0; i < L; ++i) {
        const int64_t p = i + W / 2;
        if (p >= span) {
            out[i] = 0.0f;
            continue;
        }
        int64_t t_lo, t_hi;
        istft_cover(p, W, H, F, t_lo, t_hi);
        float num = 0.0f;
        double env = 0.0;
        for (int64_t t = t_lo; t <= t_hi; ++t) {
            num = num + y[(size_t)(t * W + (p - t * H))];
            const double w = (double)w32[p - t * H];
            env = env + w * w;
        }
        const float v = num / (float)env;
        out[i] = v != v ? __builtin_bit_cast(float, kQuietNan) : v;
    }
}

}  // namespace

}  // namespace nc

using namespace nc;

extern "C" int64_t nc_audio_istft_len(int64_t frames, int32_t W, int32_t H) {
    if (W < 2 || H < 1 || frames < 1) return -1;
    return istft_default_len(frames, H);
}

extern "C" nc_status nc_op_logf(const float* x, int64_t n, float* y) {
    return guard([&] {
        if (!x || !y || n < 0) fail(NC_EINVAL, "null pointer or negative count");
        for (int64_t i = 0; i < n; ++i) y[i] = nc_logf(x[i]);
    });
}

extern "C" nc_status nc_audio_idft_basis(int32_t W, int32_t window, float* T) {
    return guard([&] {
        if (!T) fail(NC_EINVAL, "null pointer");
        quality_check_window(W, 1, window);
        build_idft_basis(W, window, T);
    });
}

extern "C" nc_status nc_audio_dct_matrix(int32_t n_mfcc, int32_t n_mels, float* dct) {
    return guard([&] {
        if (!dct) fail(NC_EINVAL, "null pointer");
        spectral_check_mfcc(n_mfcc, n_mels, 1.0f);
        build_dct_matrix(n_mfcc, n_mels, dct);
    });
}

extern "C" nc_status nc_audio_mask_freq_bins(int32_t sample_rate, int32_t nbins, float fmin_hz, float fmax_hz, int32_t* k_lo, int32_t* k_hi) {
    return guard([&] {
        if (!k_lo || !k_hi) fail(NC_EINVAL, "null pointer");
        if (sample_rate <= 0) fail(NC_EINVAL, "sample rate must be positive");
        if (nbins < 1 || nbins > 1025) fail(NC_EINVAL, "nbins = %d is not in [1, 1025]", nbins);
        if (!(fmin_hz < fmax_hz)) fail(NC_EINVAL, "the minimum frequency must be below the maximum frequency");
        const double top = (double)(sample_rate / 2);   // the reference's INTEGER sample_rate / 2
        auto bin = [&](int64_t k) { return nbins == 1 ? 0.0 : (double)k * top / (double)(nbins - 1); };
        *k_lo = (int32_t)spectral_first_at_least(nbins, (double)fmin_hz, bin);
        *k_hi = (int32_t)spectral_first_at_least(nbins, (double)fmax_hz, bin);
    });
}

extern "C" nc_status nc_audio_mask_time_frames(float duration, int64_t frames, float tmin_s, float tmax_s, int64_t* t_lo, int64_t* t_hi) {
    return guard([&] {
        if (!t_lo || !t_hi) fail(NC_EINVAL, "null pointer");
        if (!(duration >= 0.0f) || !std::isfinite(duration)) fail(NC_EINVAL, "the duration must be finite and not negative");
        if (frames < 1 || frames > ((int64_t)1 << 40)) fail(NC_EINVAL, "frames = %lld is not in [1, 2^40]", (long long)frames);
        if (!(tmin_s < tmax_s)) fail(NC_EINVAL, "the minimum time must be below the maximum time");
        auto bin = [&](int64_t t) { return frames == 1 ? 0.0 : (double)t * (double)duration / (double)(frames - 1); };
        *t_lo = spectral_first_at_least(frames, (double)tmin_s, bin);
        *t_hi = spectral_first_at_least(frames, (double)tmax_s, bin);
    });
}

extern "C" nc_status nc_audio_istft_host(const float* spec_c64, int32_t B, const int64_t* spec_off, const int64_t* frames, int32_t W, int32_t H,
                                         int32_t window, float* out, const int64_t* out_off, const int64_t* length) {
    return guard([&] {
        const std::vector<int64_t> len = istft_check_rows(spec_c64, B, spec_off, frames, W, H, window, out, out_off, length);
        std::vector<float> T((size_t)W * (W + 2)), w32((size_t)W);
        build_idft_basis(W, window, T.data());
        build_window32(W, window, w32.data());
        for (int b = 0; b < B; ++b) istft_row(spec_c64 + 2 * spec_off[b], frames[b], W, H, T.data(), w32.data(), out + out_off[b], len[(size_t)b]);
    });
}

extern "C" nc_status nc_audio_spec_fill_host(float* spec_c64, int32_t B, const int64_t* spec_off, const int64_t* frames, int32_t nbins,
                                             const int32_t* k_lo, const int32_t* k_hi, const int64_t* t_lo, const int64_t* t_hi, float val) {
    return guard([&] {
        spectral_check_fill(spec_c64, B, spec_off, frames, nbins, k_lo, k_hi, t_lo, t_hi);
        float re, im;
        spectral_fill_value(val, &re, &im);
        for (int b = 0; b < B; ++b)
            for (int k = k_lo[b]; k < k_hi[b]; ++k)
                for (int64_t t = t_lo[b]; t < t_hi[b]; ++t) {
                    float* o = spec_c64 + 2 * (spec_off[b] + (int64_t)k * frames[b] + t);
                    o[0] = re;
                    o[1] = im;
                }
    });
}

extern "C" nc_status nc_audio_mfcc_host(const float* pcm, int32_t B, const int64_t* off, const int64_t* n, int32_t sample_rate, int32_t W, int32_t H,
                                        int32_t n_mels, float fmin, float fmax, int32_t n_mfcc, float log_offset, float* out, const int64_t* out_off) {
    return guard([&] {
        if (!pcm || !out || !off || !n || !out_off) fail(NC_EINVAL, "null pointer");
        spectral_check_mfcc(n_mfcc, n_mels, log_offset);
        if (B < 1 || B > 32767) fail(NC_EINVAL, "B = %d is not in [1, 32767]", B);
        quality_check_window(W, H, NC_WINDOW_HANN);
        std::vector<float> dct((size_t)n_mfcc * n_mels);
        build_dct_matrix(n_mfcc, n_mels, dct.data());
        for (int b = 0; b < B; ++b) {
            if (out_off[b] < 0) fail(NC_EINVAL, "row %d has a negative offset", b);
            const int64_t zero = 0;
            if (n[b] <= W / 2) fail(NC_EINVAL, "row %d has %lld samples: reflect padding of window %d needs more than %d", b, (long long)n[b], W, W / 2);
            const int64_t F = 1 + n[b] / H;
            std::vector<float> mel((size_t)(n_mels * F));
            const nc_status st = nc_audio_mel_spectrogram_host(pcm, 1, off + b, n + b, sample_rate, W, H, n_mels, fmin, fmax, mel.data(), &zero);
            if (st != NC_OK) fail(st, "%s", nc_last_error());
            for (int c = 0; c < n_mfcc; ++c)
                for (int64_t t = 0; t < F; ++t) {
                    float acc = 0.0f;
                    for (int m = 0; m < n_mels; ++m) {
                        const float v = mel[(size_t)(m * F + t)] + log_offset;
                        const float l = finite32(v) ? nc_logf(v) : __builtin_bit_cast(float, kQuietNan);
                        acc = nc_fma(dct[(size_t)c * n_mels + m], l, acc);
                    }
                    out[out_off[b] + (int64_t)c * F + t] = acc != acc ? __builtin_bit_cast(float, kQuietNan) : acc;
                }
        }
    });
}
