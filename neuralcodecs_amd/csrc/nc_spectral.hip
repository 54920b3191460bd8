// Inverse STFT, spectral masks and MFCC on the device (include/nc_mi355x.h "inverse STFT, spectral masks, MFCC").  The
// arithmetic of every output element is the one chain the header states, so the results equal the serial host twin (nc_spectral_host.hip)
// bit for bit; the two units share nc_math.h, the host table builders and the argument checks (nc_spectral.h) and nothing else.
//
// istft_mfma_kernel: y[t][n] = sum_j T[n][j] Xflat[j][t] as D[16 samples n][16 frames t] = A B with v_mfma_f32_16x16x4_f32, whose result is
// the k-ordered fmaf chain.  A workgroup (4 waves) serves 16 frames x up to 256 samples; a wave holds up to four 16-sample tiles, ONE
// accumulator each, and walks j = 0 .. W + 1 in ascending order: no chain is split.  The B operand is the spectrogram itself, read where
// it lies: lanes 0..15 of one k-quarter take 16 consecutive frames of one part (re or im) of one bin, stride two floats, and the quarter
// beside them the other part of the same bin, so the two quarters together read one whole 128-byte stretch and an instruction two of
// them (bins 2s and 2s + 1); nothing is staged, the four waves of a workgroup read the same lines.  The A operand comes straight from the
// cached table image, stored per sample n as four runs [j % 4][j / 4], each padded with +0 to W/4 + 4 words, so that a lane's taps of four
// consecutive instructions are one 16-byte load.  W + 2 = 4 (W/4) + 2: the last instruction has two live k lanes (j = W, W + 1); the other
// two multiply the table's +0 by a literal +0 and read nothing.  The two extra terms fmaf(+0, +0, acc) can turn an accumulator that is -0
// into +0; the sign of a zero frame sample never reaches a result, because the overlap-add sum starts from +0.
// A lane's four results are four consecutive samples of one frame: one 16-byte store into the frame scratch [frames][W].
// istft_gather_kernel: one thread per output sample, the frames that cover it ascending: the binary32 sum of the frame samples, the
// binary64 sum of the squared window, one division.
#include "nc_devcall.h"
#include "nc_frag.h"
#include "nc_guard.h"
#include "nc_math.h"
#include "nc_spectral.h"

namespace nc {

namespace {

constexpr int kFramesPerBlock = 16, kTilesPerWave = 4, kTilesPerBlock = 16;
constexpr uint32_t kQuietNan = 0x7fc00000u;

struct IstftRow {
    const float* spec;   // [W/2+1][frames] (re, im)
    float* out;
    int64_t frames, length;
    int64_t y_off;       // floats into the frame scratch, within the row's group
};

struct FillRow {
    float* spec;
    int64_t frames, t_lo, t_hi;
    int32_t k_lo, k_hi;
};

struct MfccRow {
    const float* mel;    // [n_mels][frames]
    float* out;          // [n_mfcc][frames]
    int64_t frames;
};

__global__ __launch_bounds__(256) void istft_mfma_kernel(const IstftRow* __restrict__ rows, const float* __restrict__ basis, int W, int Q4,
                                                         float* __restrict__ y) {
    const IstftRow r = rows[blockIdx.z];
    const int64_t t0 = (int64_t)blockIdx.x * kFramesPerBlock;
    if (t0 >= r.frames) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rr = lane & 15, kq = lane >> 4;
    const int tiles = W >> 4, tile0 = blockIdx.y * kTilesPerBlock + wave;
    if (tile0 >= tiles) return;   // (no barrier in this kernel)
    const int64_t t = t0 + rr;
    const int64_t tc = t < r.frames ? t : r.frames - 1;   // a column behind the last frame reads the last frame and is never stored
    const float* bp = r.spec + 2 * ((int64_t)(kq >> 1) * r.frames + tc) + (kq & 1);
    const int64_t bstep = 4 * r.frames;                   // two bins per instruction
    const float* ap[kTilesPerWave];
#pragma unroll
    for (int i = 0; i < kTilesPerWave; ++i) {
        const int tile = tile0 + 4 * i;
        ap[i] = basis + ((size_t)(16 * (tile < tiles ? tile : tile0) + rr) * 4 + (size_t)kq) * (size_t)Q4;
    }
    f32x4_t acc[kTilesPerWave];
#pragma unroll
    for (int i = 0; i < kTilesPerWave; ++i) acc[i] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};
    const int Wq = W >> 2;
    for (int s = 0; s < Wq; s += 4) {
        f32x4_t a[kTilesPerWave];
#pragma unroll
        for (int i = 0; i < kTilesPerWave; ++i) a[i] = *reinterpret_cast<const f32x4_t*>(ap[i] + s);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float b = bp[(int64_t)(s + u) * bstep];
#pragma unroll
            for (int i = 0; i < kTilesPerWave; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][u], b, acc[i], 0, 0, 0);
        }
    }
    {   // j = W, W + 1 in k lanes 0 and 1 (bin W/2); lanes 2 and 3 would be bin W/2 + 1: an exact zero, nothing read
        const float b = kq < 2 ? bp[(int64_t)Wq * bstep] : 0.0f;
#pragma unroll
        for (int i = 0; i < kTilesPerWave; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[i][Wq], b, acc[i], 0, 0, 0);
    }
    if (t >= r.frames) return;
#pragma unroll
    for (int i = 0; i < kTilesPerWave; ++i) {
        const int tile = tile0 + 4 * i;
        if (tile < tiles) *reinterpret_cast<f32x4_t*>(y + r.y_off + t * W + 16 * tile + 4 * kq) = acc[i];
    }
}

__global__ __launch_bounds__(256) void istft_gather_kernel(const IstftRow* __restrict__ rows, const float* __restrict__ y, const float* __restrict__ w32,
                                                           int W, int H) {
    const IstftRow r = rows[blockIdx.y];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= r.length) return;
    const int64_t p = i + (W >> 1);
    if (p >= (int64_t)W + (int64_t)H * (r.frames - 1)) {
        r.out[i] = 0.0f;
        return;
    }
    const int64_t first = p < W ? 0 : (p - W) / H + 1;
    int64_t last = p / H;
    last = last < r.frames - 1 ? last : r.frames - 1;
    const float* yr = y + r.y_off;
    float num = 0.0f;
    double env = 0.0;
    for (int64_t t = first; t <= last; ++t) {
        const int64_t n = p - t * H;
        num = num + yr[t * W + n];
        const double w = (double)w32[n];
        env = env + w * w;
    }
    const float v = num / (float)env;
    r.out[i] = v != v ? __builtin_bit_cast(float, kQuietNan) : v;
}

__global__ __launch_bounds__(256) void spec_fill_kernel(const FillRow* __restrict__ rows, float re, float im) {
    const FillRow r = rows[blockIdx.z];
    const int64_t t = r.t_lo + (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int k = r.k_lo + (int)blockIdx.y;
    if (t >= r.t_hi || k >= r.k_hi) return;
    float* o = r.spec + 2 * ((int64_t)k * r.frames + t);
    o[0] = re;
    o[1] = im;
}

// mfcc[c][t]: one fmaf chain over the bands ascending.  One thread per (coefficient, frame); the frames of a band are consecutive words.
__global__ __launch_bounds__(256) void mfcc_kernel(const MfccRow* __restrict__ rows, const float* __restrict__ dct, int M, float log_offset) {
    const MfccRow r = rows[blockIdx.z];
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= r.frames) return;
    const int c = blockIdx.y;
    const float* d = dct + (size_t)c * M;
    float acc = 0.0f;
    for (int m = 0; m < M; ++m) {
        const float v = r.mel[(int64_t)m * r.frames + t] + log_offset;
        const float l = finite32(v) ? nc_logf(v) : __builtin_bit_cast(float, kQuietNan);
        acc = nc_fma(d[m], l, acc);
    }
    r.out[(int64_t)c * r.frames + t] = acc != acc ? __builtin_bit_cast(float, kQuietNan) : acc;
}

// ---- per-device state: the cached tables and the workspace beside the call scaffold (nc_devcall.h) ----------------------------------------
struct SpectralDev {
    DevCall call;
    std::map<std::pair<int, int>, DevBuf> basis;    // (W, window) -> [W][4][W/4 + 4]
    std::map<std::pair<int, int>, DevBuf> window;   // (W, window) -> w32[W]
    std::map<std::pair<int, int>, DevBuf> dct;      // (n_mfcc, n_mels) -> [n_mfcc][n_mels]
    DevBuf y, mel, in, out;
    int64_t cap = kIstftDefaultCap;                 // bytes of frame scratch per group of rows
};

PerDevice<SpectralDev> g_spectral;

int run_of(int W) { return W / 4 + 4; }

const float* basis_on(SpectralDev& d, int W, int window) {
    return cached_table(d.basis[{W, window}], [&](DevBuf& t) {
        const int J = W + 2, Q4 = run_of(W);
        std::vector<float> T((size_t)W * J), img((size_t)W * 4 * Q4, 0.0f);   // the tail of every run stays +0
        build_idft_basis(W, window, T.data());
        for (int n = 0; n < W; ++n)
            for (int j = 0; j < J; ++j) img[((size_t)n * 4 + (size_t)(j & 3)) * Q4 + (size_t)(j >> 2)] = T[(size_t)n * J + j];
        fill_table(t, img.data(), img.size());
    }).as<float>();
}

const float* window_on(SpectralDev& d, int W, int window) {
    return cached_table(d.window[{W, window}], [&](DevBuf& t) {
        std::vector<float> w((size_t)W);
        build_window32(W, window, w.data());
        fill_table(t, w.data(), w.size());
    }).as<float>();
}

const float* dct_on(SpectralDev& d, int n_mfcc, int n_mels) {
    return cached_table(d.dct[{n_mfcc, n_mels}], [&](DevBuf& t) {
        std::vector<float> m((size_t)n_mfcc * n_mels);
        build_dct_matrix(n_mfcc, n_mels, m.data());
        fill_table(t, m.data(), m.size());
    }).as<float>();
}

// The rows of a call run in groups whose frame scratch stays under the cap; a row above the cap is a group of its own.  A sample's value
// depends on nothing but its row, so the grouping changes no bit.  spec_at / out_at: FLOAT offsets into spec / out.
void run_istft(SpectralDev& d, const float* spec, int B, const int64_t* spec_at, const int64_t* frames, int W, int H, int window, float* out,
               const int64_t* out_at, const int64_t* len, hipStream_t s) {
    std::vector<IstftRow> rows((size_t)B);
    std::vector<int> group_end;
    int64_t in_group = 0, max_group = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t need = frames[b] * W;
        if (in_group > 0 && (in_group + need) * (int64_t)sizeof(float) > d.cap) {
            group_end.push_back(b);
            in_group = 0;
        }
        rows[(size_t)b] = IstftRow{spec + spec_at[b], out + out_at[b], frames[b], len[b], in_group};
        in_group += need;
        max_group = in_group > max_group ? in_group : max_group;
    }
    group_end.push_back(B);
    d.call.begin(s);
    d.y.reserve((size_t)max_group * sizeof(float));
    const float* T = basis_on(d, W, window);
    const float* w32 = window_on(d, W, window);
    const IstftRow* d_rows = d.call.upload(rows, s);
    int b0 = 0;
    for (int b1 : group_end) {
        int64_t max_frames = 0, max_len = 0;
        for (int b = b0; b < b1; ++b) {
            max_frames = frames[b] > max_frames ? frames[b] : max_frames;
            max_len = len[b] > max_len ? len[b] : max_len;
        }
        if (max_len > 0) {   // a group that writes nothing needs no frames
            const unsigned gx = grid_of(max_frames, kFramesPerBlock, 0x7fffffff);
            hipLaunchKernelGGL(istft_mfma_kernel, dim3(gx, (unsigned)((W / 16 + kTilesPerBlock - 1) / kTilesPerBlock), (unsigned)(b1 - b0)), dim3(256), 0, s,
                               d_rows + b0, T, W, run_of(W), d.y.as<float>());
            hipLaunchKernelGGL(istft_gather_kernel, dim3(grid_of(max_len, 256, 0xffffff), (unsigned)(b1 - b0)), dim3(256), 0, s, d_rows + b0,
                               d.y.as<float>(), w32, W, H);
        }
        b0 = b1;
    }
    d.call.end(s);
}

}  // namespace

}  // namespace nc

using namespace nc;

extern "C" nc_status nc_audio_istft_workspace(int device_index, int64_t set_bytes, int64_t* cap_bytes) {
    return guard([&] {
        if (set_bytes < -1) fail(NC_EINVAL, "the cap is a number of bytes, 0 (keep) or -1 (the default)");
        g_spectral.locked(device_index, [&](SpectralDev& d) {
            if (set_bytes == -1) d.cap = kIstftDefaultCap;
            if (set_bytes > 0) d.cap = set_bytes;
            if (cap_bytes) *cap_bytes = d.cap;
        });
    });
}

extern "C" nc_status nc_audio_istft_dev(int device_index, const float* spec_c64, int32_t B, const int64_t* spec_off, const int64_t* frames, int32_t W,
                                        int32_t H, int32_t window, float* out, const int64_t* out_off, const int64_t* length, void* hip_stream) {
    return guard([&] {
        const std::vector<int64_t> len = istft_check_rows(spec_c64, B, spec_off, frames, W, H, window, out, out_off, length);
        std::vector<int64_t> at((size_t)B);
        for (int b = 0; b < B; ++b) at[(size_t)b] = 2 * spec_off[b];
        g_spectral.locked(device_index, [&](SpectralDev& d) {
            run_istft(d, spec_c64, B, at.data(), frames, W, H, window, out, out_off, len.data(), static_cast<hipStream_t>(hip_stream));
        });
    });
}

extern "C" nc_status nc_audio_istft(int device_index, const float* spec_c64, int32_t B, const int64_t* spec_off, const int64_t* frames, int32_t W,
                                    int32_t H, int32_t window, float* out, const int64_t* out_off, const int64_t* length) {
    return guard([&] {
        const std::vector<int64_t> len = istft_check_rows(spec_c64, B, spec_off, frames, W, H, window, out, out_off, length);
        std::vector<int64_t> words((size_t)B), src((size_t)B);
        for (int b = 0; b < B; ++b) {
            words[(size_t)b] = 2 * (int64_t)(W / 2 + 1) * frames[b];
            src[(size_t)b] = 2 * spec_off[b];
        }
        g_spectral.locked(device_index, [&](SpectralDev& d) {
            // HOST rows -> the device staging buffers, every row at a multiple of four elements
            const PackedRows pin(B, words.data(), 1, 4), pout(B, len.data(), 1, 4);
            pin.copy_in(d.in, spec_c64, src.data());
            pout.reserve(d.out);
            run_istft(d, d.in.as<float>(), B, pin.at.data(), frames, W, H, window, d.out.as<float>(), pout.at.data(), len.data(), nullptr);
            NC_HIP(hipStreamSynchronize(nullptr));
            pout.copy_out(d.out, out, out_off);
        });
    });
}

extern "C" nc_status nc_audio_spec_fill_dev(int device_index, float* spec_c64, int32_t B, const int64_t* spec_off, const int64_t* frames,
                                            int32_t nbins, const int32_t* k_lo, const int32_t* k_hi, const int64_t* t_lo, const int64_t* t_hi,
                                            float val, void* hip_stream) {
    return guard([&] {
        spectral_check_fill(spec_c64, B, spec_off, frames, nbins, k_lo, k_hi, t_lo, t_hi);
        float re, im;
        spectral_fill_value(val, &re, &im);
        std::vector<FillRow> rows((size_t)B);
        int64_t max_t = 0;
        int max_k = 0;
        for (int b = 0; b < B; ++b) {
            rows[(size_t)b] = FillRow{spec_c64 + 2 * spec_off[b], frames[b], t_lo[b], t_hi[b], k_lo[b], k_hi[b]};
            if (t_hi[b] > t_lo[b] && k_hi[b] > k_lo[b]) {
                max_t = t_hi[b] - t_lo[b] > max_t ? t_hi[b] - t_lo[b] : max_t;
                max_k = k_hi[b] - k_lo[b] > max_k ? k_hi[b] - k_lo[b] : max_k;
            }
        }
        if (max_k == 0) return;   // every rectangle is empty
        g_spectral.locked(device_index, [&](SpectralDev& d) {
            hipStream_t s = static_cast<hipStream_t>(hip_stream);
            const unsigned gx = grid_of(max_t, 256, 0x7fffffff);
            d.call.begin(s);
            const FillRow* d_rows = d.call.upload(rows, s);
            hipLaunchKernelGGL(spec_fill_kernel, dim3(gx, (unsigned)max_k, (unsigned)B), dim3(256), 0, s, d_rows, re, im);
            d.call.end(s);
        });
    });
}

extern "C" nc_status nc_audio_mfcc_dev(int device_index, const float* pcm, int32_t B, const int64_t* off, const int64_t* n, int32_t sample_rate,
                                       int32_t W, int32_t H, int32_t n_mels, float fmin, float fmax, int32_t n_mfcc, float log_offset, float* out,
                                       const int64_t* out_off, void* hip_stream) {
    return guard([&] {
        if (!pcm || !out || !off || !n || !out_off) fail(NC_EINVAL, "null pointer");
        spectral_check_mfcc(n_mfcc, n_mels, log_offset);
        quality_check_window(W, H, NC_WINDOW_HANN);
        const int64_t* offs[2] = {off, out_off};
        quality_check_rows(B, offs, 2, n, &W, 1);
        std::vector<int64_t> mel_at((size_t)B);
        int64_t mel_floats = 0, max_frames = 0;
        for (int b = 0; b < B; ++b) {
            const int64_t F = 1 + n[b] / H;
            mel_at[(size_t)b] = mel_floats;
            mel_floats += F * n_mels;
            max_frames = F > max_frames ? F : max_frames;
        }
        g_spectral.locked(device_index, [&](SpectralDev& d) {
            hipStream_t s = static_cast<hipStream_t>(hip_stream);
            const unsigned gx = grid_of(max_frames, 256, 0x7fffffff);
            d.call.begin(s);   // first: the mel scratch is written below, after the previous call on whichever stream has read it
            d.mel.reserve((size_t)mel_floats * sizeof(float));
            const nc_status st = nc_audio_mel_spectrogram_dev(device_index, pcm, B, off, n, sample_rate, W, H, n_mels, fmin, fmax, d.mel.as<float>(),
                                                              mel_at.data(), hip_stream);
            if (st != NC_OK) fail(st, "%s", nc_last_error());
            std::vector<MfccRow> rows((size_t)B);
            for (int b = 0; b < B; ++b) rows[(size_t)b] = MfccRow{d.mel.as<float>() + mel_at[(size_t)b], out + out_off[b], 1 + n[b] / H};
            const float* dct = dct_on(d, n_mfcc, n_mels);
            const MfccRow* d_rows = d.call.upload(rows, s);
            hipLaunchKernelGGL(mfcc_kernel, dim3(gx, (unsigned)n_mfcc, (unsigned)B), dim3(256), 0, s, d_rows, dct, n_mels, log_offset);
            d.call.end(s);
        });
    });
}
