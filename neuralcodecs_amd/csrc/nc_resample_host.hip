// Band-limited resampling as plain serial C++ on host memory (include/nc_mi355x.h "band-limited resampling"):
// nc_audio_resample_sinc_host and the handle-less queries (_len, _geom, _table).  A product call (a CPU caller; a caller checking a device
// result) and the bit judge of the kernels in nc_resample.hip: written apart from them as loops over rows, output samples and taps,
// sharing nc_math.h (nc_fma), the table builder and the checks of nc_resample.h, and nothing else.  Built with -ffp-contract=off like
// every unit.
#include "nc_guard.h"
#include "nc_math.h"
#include "nc_resample.h"

namespace nc {

namespace {

// y[0..n_out) of one row: one k-ascending chain per output, the edge sample repeated on either side
void resample_row(const ResampleGeom& q, const float* h, const float* x, int64_t n, float* y) {
    const int64_t n_out = resample_len(n, q.U, q.D);
    for (int64_t o = 0; o < n_out; ++o) {
        const int64_t m = o / q.U, i = o % q.U;
        const float* hi = h + i * q.K4;
        float acc = 0.0f;
        for (int64_t k = 0; k < q.K4; ++k) {
            int64_t j = m * q.D + k - q.W;
            j = j < 0 ? 0 : (j > n - 1 ? n - 1 : j);
            acc = nc_fma(hi[k], x[j], acc);
        }
        y[o] = acc != acc ? __builtin_bit_cast(float, 0x7fc00000u) : acc;
    }
}

}  // namespace

}  // namespace nc

using namespace nc;

extern "C" int64_t nc_audio_resample_sinc_len(int64_t n_in, int32_t src, int32_t dst) {
    if (src < 1 || dst < 1 || n_in < 0 || n_in > kResampleMaxLen) return -1;
    const int64_t g = resample_gcd(src, dst);
    return resample_len(n_in, dst / g, src / g);
}

extern "C" nc_status nc_audio_resample_sinc_geom(int32_t src, int32_t dst, const nc_resample_cfg* cfg, int32_t* U, int32_t* D, int32_t* W, int32_t* K,
                                                 int32_t* K4) {
    return guard([&] {
        if (!U || !D || !W || !K || !K4) fail(NC_EINVAL, "null pointer");
        const ResampleGeom q = resample_geom(src, dst, cfg);
        *U = (int32_t)q.U;
        *D = (int32_t)q.D;
        *W = (int32_t)q.W;
        *K = (int32_t)q.K;
        *K4 = (int32_t)q.K4;
    });
}

extern "C" nc_status nc_audio_resample_sinc_table(int32_t src, int32_t dst, const nc_resample_cfg* cfg, float* h) {
    return guard([&] {
        if (!h) fail(NC_EINVAL, "null pointer");
        const ResampleGeom q = resample_geom(src, dst, cfg);
        std::vector<float> t;
        build_resample_table(q, t);
        std::copy(t.begin(), t.end(), h);
    });
}

extern "C" nc_status nc_audio_resample_sinc_host(const float* pcm, int32_t R, const int64_t* off, const int64_t* n, int32_t src, int32_t dst,
                                                 const nc_resample_cfg* cfg, float* out, const int64_t* out_off) {
    return guard([&] {
        const ResampleGeom q = resample_geom(src, dst, cfg);
        resample_check_rows(pcm, R, off, n, q, src == dst, out, out_off);
        if (src == dst) {
            for (int r = 0; r < R; ++r) std::copy(pcm + off[r], pcm + off[r] + n[r], out + out_off[r]);
            return;
        }
        std::vector<float> h;
        build_resample_table(q, h);
        for (int r = 0; r < R; ++r) resample_row(q, h.data(), pcm + off[r], n[r], out + out_off[r]);
    });
}
