// Spectrogram synthesis and editing (include/nc_mi355x.h "inverse STFT, spectral masks, MFCC"): what the device unit
// (nc_spectral.hip) and the serial host twin (nc_spectral_host.hip) share besides nc_math.h -- the argument checks, the host table builders,
// the envelope rule and the index helpers of the masks.  Nothing of the arithmetic on spectrogram bins or samples lives here: each unit has
// its own.
#pragma once
#include <cmath>
#include <vector>

#include "nc_common.h"
#include "nc_quality.h"

namespace nc {

constexpr int64_t kIstftMaxLen = ((int64_t)1 << 31) - 256;      // output samples of one row that one launch covers
constexpr int64_t kIstftMaxRowScratch = (int64_t)2 << 30;       // bytes of frame scratch (frames x W floats) one row may need
constexpr int64_t kIstftDefaultCap = (int64_t)256 << 20;        // bytes of frame scratch one group of rows may need (nc_audio_istft_workspace)
constexpr double kNolaFloor = 1e-11;                            // torch.istft's bound on the window envelope

// w32[W]: the window in binary64, rounded once
inline void build_window32(int W, int window, float* w) {
    const double two_pi = 2.0 * 3.14159265358979323846;
    for (int n = 0; n < W; ++n) w[n] = (float)(window == NC_WINDOW_ONES ? 1.0 : 0.5 - 0.5 * std::cos(two_pi * (double)n / (double)W));
}

// T[W][W + 2] as the header defines it; the imaginary columns of k = 0 and k = W/2 are exactly +0
inline void build_idft_basis(int W, int window, float* T) {
    const double two_pi = 2.0 * 3.14159265358979323846;
    const int J = W + 2;
    for (int n = 0; n < W; ++n) {
        const double w = window == NC_WINDOW_ONES ? 1.0 : 0.5 - 0.5 * std::cos(two_pi * (double)n / (double)W);
        for (int k = 0; k <= W / 2; ++k) {
            const double ck = (k == 0 || k == W / 2) ? 1.0 : 2.0;
            const double ang = two_pi * (double)((k * n) % W) / (double)W;
            T[(size_t)n * J + 2 * k] = (float)(w * ck * std::cos(ang) / (double)W);
            T[(size_t)n * J + 2 * k + 1] = (k == 0 || k == W / 2) ? 0.0f : (float)(-w * ck * std::sin(ang) / (double)W);
        }
    }
}

// dct[n_mfcc][n_mels]: the orthonormal DCT-II in binary64, rounded once
inline void build_dct_matrix(int n_mfcc, int n_mels, float* dct) {
    const double pi = 3.14159265358979323846;
    const double scale = std::sqrt(2.0 / (double)n_mels), first = 1.0 / std::sqrt(2.0);
    for (int c = 0; c < n_mfcc; ++c)
        for (int m = 0; m < n_mels; ++m) {
            const double v = std::cos(pi * (double)c * (double)(2 * m + 1) / (double)(2 * n_mels)) * scale;
            dct[(size_t)c * n_mels + m] = (float)(c == 0 ? v * first : v);
        }
}

inline void spectral_check_mfcc(int n_mfcc, int n_mels, float log_offset) {
    if (n_mels < 1 || n_mels > 512) fail(NC_EINVAL, "n_mels = %d is not in [1, 512]", n_mels);
    if (n_mfcc < 1 || n_mfcc > n_mels) fail(NC_EINVAL, "n_mfcc = %d is not in [1, n_mels = %d]", n_mfcc, n_mels);
    if (!(log_offset >= 1.17549435e-38f) || !std::isfinite(log_offset)) fail(NC_EINVAL, "log_offset must be a finite positive normal number");
}

// H (frames - 1): what torch.istft returns with center = true and no length
inline int64_t istft_default_len(int64_t frames, int H) { return (int64_t)H * (frames - 1); }

// the frames that cover padded position p: t_lo .. t_hi (empty where t_lo > t_hi)
inline void istft_cover(int64_t p, int W, int H, int64_t frames, int64_t& t_lo, int64_t& t_hi) {
    t_lo = p < W ? 0 : (p - W) / H + 1;
    t_hi = p / H < frames - 1 ? p / H : frames - 1;
}

// the binary64 envelope at padded position p, t ascending
inline double istft_envelope(const float* w32, int64_t p, int W, int H, int64_t frames) {
    int64_t t_lo, t_hi;
    istft_cover(p, W, H, frames, t_lo, t_hi);
    double e = 0.0;
    for (int64_t t = t_lo; t <= t_hi; ++t) {
        const double w = (double)w32[p - t * H];
        e = e + w * w;
    }
    return e;
}

// The rows of an inverse transform, checked and resolved: len[b] is the number of samples row b writes.  NOLA: every covered output sample
// has an envelope above 1e-11.  The envelope of positions W <= p < H frames is periodic in p with period H (the same terms in the same
// order), so one period stands for them all.
inline std::vector<int64_t> istft_check_rows(const float* spec, int B, const int64_t* spec_off, const int64_t* frames, int W, int H, int window,
                                              const float* out, const int64_t* out_off, const int64_t* length) {
    if (!spec || !out || !spec_off || !frames || !out_off) fail(NC_EINVAL, "null pointer");
    quality_check_window(W, H, window);
    if (B < 1 || B > 32767) fail(NC_EINVAL, "B = %d is not in [1, 32767]", B);
    std::vector<float> w32((size_t)W);
    build_window32(W, window, w32.data());
    std::vector<int64_t> len((size_t)B);
    for (int b = 0; b < B; ++b) {
        if (spec_off[b] < 0 || out_off[b] < 0) fail(NC_EINVAL, "row %d has a negative offset", b);
        if (frames[b] < 1) fail(NC_EINVAL, "row %d has %lld frames: at least 1", b, (long long)frames[b]);
        if (frames[b] > kIstftMaxRowScratch / (4 * (int64_t)W)) fail(NC_EINVAL, "row %d has too many frames for one call", b);
        const int64_t L = length ? length[b] : 0;
        if (L < 0) fail(NC_EINVAL, "row %d has a negative length", b);
        if (L > kIstftMaxLen) fail(NC_EINVAL, "row %d is too long for one launch", b);
        len[(size_t)b] = L == 0 ? istft_default_len(frames[b], H) : L;
        const int64_t F = frames[b], span = (int64_t)W + (int64_t)H * (F - 1);
        const int64_t p_end = W / 2 + len[(size_t)b] < span ? W / 2 + len[(size_t)b] : span;
        for (int64_t p = W / 2; p < p_end; ++p) {
            if (p >= (int64_t)W + H && p < (int64_t)H * F) {   // interior: env(p) == env(p - H)
                p = (int64_t)H * F - 1;
                continue;
            }
            if (!(istft_envelope(w32.data(), p, W, H, F) > kNolaFloor))
                fail(NC_EINVAL, "row %d: the window envelope at sample %lld is not above 1e-11 (NOLA)", b, (long long)(p - W / 2));
        }
    }
    return len;
}

// val exp(i val) in binary64, rounded once
inline void spectral_fill_value(float val, float* re, float* im) {
    if (!std::isfinite(val)) fail(NC_EINVAL, "the fill value must be finite");
    const double v = (double)val;
    *re = (float)(v * std::cos(v));
    *im = (float)(v * std::sin(v));
}

inline void spectral_check_fill(const float* spec, int B, const int64_t* spec_off, const int64_t* frames, int nbins, const int32_t* k_lo,
                                const int32_t* k_hi, const int64_t* t_lo, const int64_t* t_hi) {
    if (!spec || !spec_off || !frames || !k_lo || !k_hi || !t_lo || !t_hi) fail(NC_EINVAL, "null pointer");
    if (B < 1 || B > 32767) fail(NC_EINVAL, "B = %d is not in [1, 32767]", B);
    if (nbins < 1 || nbins > 1025) fail(NC_EINVAL, "nbins = %d is not in [1, 1025]", nbins);
    for (int b = 0; b < B; ++b) {
        if (spec_off[b] < 0) fail(NC_EINVAL, "row %d has a negative offset", b);
        if (frames[b] < 1 || frames[b] > ((int64_t)1 << 40)) fail(NC_EINVAL, "row %d has %lld frames", b, (long long)frames[b]);
        if (k_lo[b] < 0 || k_lo[b] > k_hi[b] || k_hi[b] > nbins) fail(NC_EINVAL, "row %d: bins [%d, %d) are not within [0, %d]", b, k_lo[b], k_hi[b], nbins);
        if (t_lo[b] < 0 || t_lo[b] > t_hi[b] || t_hi[b] > frames[b])
            fail(NC_EINVAL, "row %d: frames [%lld, %lld) are not within [0, %lld]", b, (long long)t_lo[b], (long long)t_hi[b], (long long)frames[b]);
    }
}

// the first index i in [0, count] with at(i) >= bound; at is non-decreasing
template <class At>
int64_t spectral_first_at_least(int64_t count, double bound, At&& at) {
    int64_t lo = 0, hi = count;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (at(mid) >= bound) hi = mid; else lo = mid + 1;
    }
    return lo;
}

}  // namespace nc
