// Round-trip quality on the device (include/nc_mi355x.h "round-trip quality"): STFT on the fp32 matrix cores, mel bands, the
// time-domain sums and the per-row finish.  The arithmetic of every output element is the one chain the header states, so the results
// equal the serial host twin (nc_quality_host.hip) bit for bit; the two units share nc_math.h, the host table builders and the argument
// checks (nc_quality.h) and nothing else.
//
// stft_mfma_kernel: D[j][t] = sum_n T[j][n] x_pad[t H + n] with v_mfma_f32_16x16x4_f32, whose result is the k-ordered fmaf chain.  Basis
// rows j interleave the bins (2k: C[k], 2k + 1: S[k]), so a lane's four accumulator registers hold (re, im) of two bins of one frame and
// the magnitude needs no exchange between lanes.  A workgroup (4 waves) serves 16 frames x 256 basis rows; blockIdx.y walks the rows.
// It stages ONE stretch of 15 H + W padded samples in LDS, reflect padding resolved while staging, and every wave reads its B operand
// (16 frames x 4 taps per instruction) out of it.  Sample i of the stretch lies at word i + 2 (i / H): frame f starts at f (H + 2), so
// the 16 frames of one tap fall into 16 distinct even banks and the tap beside it (lanes +16) into the odd ones -- ds_read_b32 serves 32
// lanes per cycle over 32 banks, conflict-free for every even H.  The A operand comes straight from the cached table, stored per row as
// four runs [n % 4][n / 4] so that a lane's taps of four consecutive instructions are one 16-byte load.
#include "nc_devcall.h"
#include "nc_frag.h"
#include "nc_guard.h"
#include "nc_math.h"
#include "nc_quality.h"

namespace nc {

namespace {

constexpr int kFramesPerBlock = 16, kRowsPerWave = 64, kRowsPerBlock = 256;

struct StftRow {
    const float* x;
    int64_t n, frames;
    int64_t c_off;     // complex elements into the complex output
    int64_t mag_off;   // floats into the magnitude scratch: [K][frames] of this row
    int64_t mel_off;   // floats into the mel output / scratch: [M][frames] of this row
    int64_t f0;        // frames of the rows before this one (frame-sum arrays)
};

struct TimeRow {
    const float* x;    // estimate
    const float* y;    // reference
    int64_t n, p0;     // first block of this row in the partial arrays
};

__device__ __forceinline__ int hop_div(int i, int H, int hshift) { return hshift >= 0 ? (i >> hshift) : (i / H); }

__global__ __launch_bounds__(256) void stft_mfma_kernel(const StftRow* __restrict__ rows, const float* __restrict__ basis, int W, int H, int hshift,
                                                        int nJ, float* __restrict__ cplx, float* __restrict__ mag) {
    extern __shared__ float xs[];
    const StftRow r = rows[blockIdx.z];
    const int64_t t0 = (int64_t)blockIdx.x * kFramesPerBlock;
    if (t0 >= r.frames) return;   // the whole workgroup: before any barrier
    const int span = (kFramesPerBlock - 1) * H + W, half = W / 2;
    const int64_t s0 = t0 * H - half;
    for (int i = threadIdx.x; i < span; i += 256) {
        int64_t p = s0 + i;
        if (p < 0) p = -p;
        if (p >= r.n) p = 2 * (r.n - 1) - p;
        float v = 0.0f;   // behind the last frame of the row: never part of a result
        if (p >= 0 && p < r.n) v = r.x[p];
        xs[i + 2 * hop_div(i, H, hshift)] = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rr = lane & 15, kq = lane >> 4;
    const int jbase = blockIdx.y * kRowsPerBlock + wave * kRowsPerWave;
    if (jbase >= nJ) return;   // (no barrier below)
    const int Wq = W >> 2;
    const float* ap[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int j = jbase + 16 * i + rr;
        j = j < nJ ? j : nJ - 1;
        ap[i] = basis + (size_t)j * W + (size_t)kq * Wq;
    }
    const int xb = rr * (H + 2);
    f32x4_t acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};
    for (int q = 0; q < Wq; q += 4) {
        f32x4_t a[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const f32x4_t*>(ap[i] + q);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int n = 4 * (q + u) + kq;
            const float b = xs[xb + n + 2 * hop_div(n, H, hshift)];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][u], b, acc[i], 0, 0, 0);
        }
    }
    const int64_t t = t0 + rr;
    if (t >= r.frames) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int j = jbase + 16 * i + 4 * kq + 2 * p;
            if (j >= nJ) continue;
            const int k = j >> 1;
            const float re = acc[i][2 * p], im = acc[i][2 * p + 1];
            if (cplx) {
                float* o = cplx + 2 * (r.c_off + (int64_t)k * r.frames + t);
                o[0] = re;
                o[1] = im;
            }
            if (mag) {
                const float a2 = re * re, b2 = im * im;
                mag[r.mag_off + (int64_t)k * r.frames + t] = sqrtf(a2 + b2);
            }
        }
    }
}

// mel[m][t]: one fmaf chain over the bins of the band's support, ascending.  One thread per (band, frame); the frames of a bin are
// consecutive words, so a wave reads and writes whole lines.
__global__ __launch_bounds__(256) void mel_apply_kernel(const StftRow* __restrict__ rows, const float* __restrict__ mag, const float* __restrict__ fb,
                                                        const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, int K, float* __restrict__ mel) {
    const StftRow r = rows[blockIdx.z];
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= r.frames) return;
    const int m = blockIdx.y;
    const float* w = fb + (size_t)m * K;
    const float* g = mag + r.mag_off + t;
    float acc = 0.0f;
    for (int k = lo[m]; k < hi[m]; ++k) acc = nc_fma(w[k], g[(int64_t)k * r.frames], acc);
    mel[r.mel_off + (int64_t)m * r.frames + t] = acc;
}

__device__ __forceinline__ float log_mel(float v, float clamp_eps) {
    const float c = v > clamp_eps ? v : clamp_eps;
    return nc_log10f(c * c);
}

// per frame of row b: the bands ascending, binary64.  rows[b] is the estimate, rows[B + b] the reference (same frame count).
__global__ __launch_bounds__(256) void mel_frame_sums_kernel(const StftRow* __restrict__ rows, int B, const float* __restrict__ mel, int M, float clamp_eps,
                                                             double* __restrict__ fs_mag, double* __restrict__ fs_log) {
    const StftRow rx = rows[blockIdx.y], ry = rows[B + blockIdx.y];
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= rx.frames) return;
    const float* X = mel + rx.mel_off + t;
    const float* Y = mel + ry.mel_off + t;
    double fm = 0.0, fl = 0.0;
    for (int m = 0; m < M; ++m) {
        const float a = X[(int64_t)m * rx.frames], b = Y[(int64_t)m * rx.frames];
        const float d = a - b;
        fm = fm + (double)__builtin_fabsf(d);
        const float dl = log_mel(a, clamp_eps) - log_mel(b, clamp_eps);
        fl = fl + (double)__builtin_fabsf(dl);
    }
    fs_mag[rx.f0 + t] = fm;
    fs_log[rx.f0 + t] = fl;
}

// row state (doubles): 0 mean x, 1 mean y, 2 sum |x - y|, 3 sum yc yc, 4 sum xc yc, 5 scale
constexpr int kRowState = 6;

// One thread per block of kQualityBlock samples, the samples ascending.  PHASE 1: sums of x, y, |x - y| and the non-finite count;
// 2: sums of yc yc and xc yc; 3: sum of (xc - scale yc)^2.  part holds three arrays of n_part doubles.
template <int PHASE>
__global__ __launch_bounds__(64) void quality_time_kernel(const TimeRow* __restrict__ trows, const double* __restrict__ state, int64_t n_part,
                                                          double* __restrict__ part, int32_t* __restrict__ part_bad) {
    const TimeRow r = trows[blockIdx.y];
    const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int64_t i0 = q * kQualityBlock;
    if (i0 >= r.n) return;
    const int64_t i1 = i0 + kQualityBlock < r.n ? i0 + kQualityBlock : r.n;
    const double* st = state + (int64_t)blockIdx.y * kRowState;
    if constexpr (PHASE == 1) {
        double sx = 0.0, sy = 0.0, sl = 0.0;
        int bad = 0;
        for (int64_t i = i0; i < i1; ++i) {
            const float x = r.x[i], y = r.y[i];
            sx = sx + (double)x;
            sy = sy + (double)y;
            const float d = x - y;
            sl = sl + (double)__builtin_fabsf(d);
            bad += (finite32(x) ? 0 : 1) + (finite32(y) ? 0 : 1);
        }
        part[r.p0 + q] = sx;
        part[n_part + r.p0 + q] = sy;
        part[2 * n_part + r.p0 + q] = sl;
        part_bad[r.p0 + q] = bad;
    } else if constexpr (PHASE == 2) {
        const double mx = st[0], my = st[1];
        double syy = 0.0, sxy = 0.0;
        for (int64_t i = i0; i < i1; ++i) {
            const double xc = (double)r.x[i] - mx, yc = (double)r.y[i] - my;
            syy = syy + yc * yc;
            sxy = sxy + xc * yc;
        }
        part[r.p0 + q] = syy;
        part[n_part + r.p0 + q] = sxy;
    } else {
        const double mx = st[0], my = st[1], scale = st[5];
        double see = 0.0;
        for (int64_t i = i0; i < i1; ++i) {
            const double xc = (double)r.x[i] - mx, yc = (double)r.y[i] - my;
            const double e = xc - scale * yc;
            see = see + e * e;
        }
        part[r.p0 + q] = see;
    }
}

struct FinishArgs {
    int32_t n_scales;
    int32_t M[NC_QUALITY_MAX_SCALES], H[NC_QUALITY_MAX_SCALES];
    int64_t fs_off[NC_QUALITY_MAX_SCALES];   // this scale's frame sums in fs_mag / fs_log
    float log_weight, mag_weight;
};

// One thread per row: the second level of every sum (blocks ascending, frames ascending), the SI-SDR formula, the mel means and the
// NaN rule.  phase 1 and 2 leave the means and the scale for the next pass over the samples; phase 3 writes the row.
__global__ __launch_bounds__(64) void quality_finish_kernel(int phase, const TimeRow* __restrict__ trows, int B, int64_t n_part,
                                                            const double* __restrict__ part, const int32_t* __restrict__ part_bad,
                                                            double* __restrict__ state, int32_t* __restrict__ row_bad, const int64_t* __restrict__ f0,
                                                            const double* __restrict__ fs_mag, const double* __restrict__ fs_log, FinishArgs fa,
                                                            nc_quality_row* __restrict__ out) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const TimeRow r = trows[b];
    const int64_t nblk = (r.n + kQualityBlock - 1) / kQualityBlock;
    double* st = state + (int64_t)b * kRowState;
    const double EPS = (double)1e-8f;
    if (phase == 1) {
        double Sx = 0.0, Sy = 0.0, Sl = 0.0;
        int64_t bad = 0;
        for (int64_t q = 0; q < nblk; ++q) {
            Sx = Sx + part[r.p0 + q];
            Sy = Sy + part[n_part + r.p0 + q];
            Sl = Sl + part[2 * n_part + r.p0 + q];
            bad += part_bad[r.p0 + q];
        }
        st[0] = Sx / (double)r.n;
        st[1] = Sy / (double)r.n;
        st[2] = Sl;
        row_bad[b] = (int32_t)(bad > 0x7fffffff ? 0x7fffffff : bad);
        return;
    }
    if (phase == 2) {
        double Syy = 0.0, Sxy = 0.0;
        for (int64_t q = 0; q < nblk; ++q) {
            Syy = Syy + part[r.p0 + q];
            Sxy = Sxy + part[n_part + r.p0 + q];
        }
        st[3] = Syy;
        st[4] = Sxy;
        st[5] = (Sxy + EPS) / (Syy + EPS);
        return;
    }
    nc_quality_row o = {};
    o.n_bad = row_bad[b];
    if (o.n_bad != 0) {
        const float nan = __builtin_nanf("");
        o.l1 = o.si_sdr_db = o.mel_distance = nan;
        for (int i = 0; i < fa.n_scales; ++i) o.mel_log[i] = o.mel_mag[i] = nan;
        out[b] = o;
        return;
    }
    double See = 0.0;
    for (int64_t q = 0; q < nblk; ++q) See = See + part[r.p0 + q];
    const double scale = st[5], Syy = st[3];
    const double target = scale * scale * Syy;
    double ratio = target / (See + EPS) + EPS;
    if (ratio > (double)3.402823466e+38f) ratio = (double)3.402823466e+38f;
    o.l1 = (float)(st[2] / (double)r.n);
    o.si_sdr_db = 10.0f * nc_log10f((float)ratio);
    double dist = 0.0;
    for (int i = 0; i < fa.n_scales; ++i) {
        const int64_t F = 1 + r.n / fa.H[i];
        const double* pm = fs_mag + fa.fs_off[i] + f0[(int64_t)i * B + b];
        const double* pl = fs_log + fa.fs_off[i] + f0[(int64_t)i * B + b];
        double Smag = 0.0, Slog = 0.0;
        for (int64_t t = 0; t < F; ++t) {
            Smag = Smag + pm[t];
            Slog = Slog + pl[t];
        }
        const double cnt = (double)((int64_t)fa.M[i] * F);
        const double mean_mag = Smag / cnt, mean_log = Slog / cnt;
        o.mel_mag[i] = (float)mean_mag;
        o.mel_log[i] = (float)mean_log;
        dist = dist + ((double)fa.log_weight * mean_log + (double)fa.mag_weight * mean_mag);
    }
    o.mel_distance = (float)dist;
    out[b] = o;
}

// ---- per-device state: the cached tables and one workspace beside the call scaffold (nc_devcall.h) --------------------------------------
struct MelKey {
    int sr, M, W;
    float fmin, fmax;
    bool operator<(const MelKey& o) const {
        if (sr != o.sr) return sr < o.sr;
        if (M != o.M) return M < o.M;
        if (W != o.W) return W < o.W;
        if (fmin != o.fmin) return fmin < o.fmin;
        return fmax < o.fmax;
    }
};
struct MelDev {
    DevBuf fb, lo, hi;
};
bool filled(const MelDev& d) { return d.fb.p != nullptr; }

struct QualityDev {
    DevCall call;
    std::map<std::pair<int, int>, DevBuf> basis;   // (W, window) -> [2 (W/2+1)][4][W/4]
    std::map<MelKey, MelDev> mel;
    DevBuf mag, melbuf, fs, part, part_bad, state, row_bad, in_est, in_ref, out_rows;
};

PerDevice<QualityDev> g_quality;

const float* basis_on(QualityDev& q, int W, int window) {
    return cached_table(q.basis[{W, window}], [&](DevBuf& d) {
        const int K = W / 2 + 1, Wq = W / 4;
        std::vector<float> C((size_t)K * W), S((size_t)K * W), T((size_t)2 * K * W);
        build_dft_basis(W, window, C.data(), S.data());
        for (int k = 0; k < K; ++k)
            for (int n = 0; n < W; ++n) {
                const size_t at = (size_t)(n & 3) * Wq + (size_t)(n >> 2);
                T[(size_t)(2 * k) * W + at] = C[(size_t)k * W + n];
                T[(size_t)(2 * k + 1) * W + at] = S[(size_t)k * W + n];
            }
        fill_table(d, T.data(), T.size());
    }).as<float>();
}

const MelDev& mel_on(QualityDev& q, int sr, int M, int W, float fmin, float fmax) {
    return cached_table(q.mel[MelKey{sr, M, W, fmin, fmax}], [&](MelDev& d) {
        const int K = W / 2 + 1;
        std::vector<float> fb((size_t)M * K);
        std::vector<int32_t> lo((size_t)M), hi((size_t)M);
        build_mel_filterbank(sr, M, W, fmin, fmax, fb.data(), lo.data(), hi.data());
        fill_table(d.fb, fb.data(), fb.size());
        fill_table(d.lo, lo.data(), lo.size());
        fill_table(d.hi, hi.data(), hi.size());
    });
}

int hop_shift(int H) {
    if (H & (H - 1)) return -1;
    int s = 0;
    while ((1 << s) < H) ++s;
    return s;
}

void launch_stft(const StftRow* rows, int R, int64_t max_frames, const float* basis, int W, int H, float* cplx, float* mag, hipStream_t s) {
    const int nJ = 2 * (W / 2 + 1);
    const int span = (kFramesPerBlock - 1) * H + W;
    const size_t lds = ((size_t)span + 2 * (size_t)(span / H) + 4) * sizeof(float);
    if (lds > 65536) fail(NC_EINVAL, "hop %d with window %d needs %zu bytes of LDS", H, W, lds);
    const int64_t gx = (max_frames + kFramesPerBlock - 1) / kFramesPerBlock;
    if (gx > 0x7fffffff) fail(NC_EINVAL, "too many frames for one launch");
    hipLaunchKernelGGL(stft_mfma_kernel, dim3((unsigned)gx, (unsigned)((nJ + kRowsPerBlock - 1) / kRowsPerBlock), (unsigned)R), dim3(256), lds, s, rows, basis, W,
                       H, hop_shift(H), nJ, cplx, mag);
}

void launch_mel(const StftRow* rows, int R, int64_t max_frames, const float* mag, const MelDev& md, int K, int M, float* mel, hipStream_t s) {
    hipLaunchKernelGGL(mel_apply_kernel, dim3((unsigned)((max_frames + 255) / 256), (unsigned)M, (unsigned)R), dim3(256), 0, s, rows, mag, md.fb.as<float>(),
                       md.lo.as<int32_t>(), md.hi.as<int32_t>(), K, mel);
}

// all launches of one metrics call on device buffers; c is resolved and checked, the rows are checked
void run_metrics(QualityDev& q, const float* ref, const int64_t* ref_off, const float* est, const int64_t* est_off, const int64_t* n, int B, int sr,
                 const nc_quality_cfg& c, nc_quality_row* out, hipStream_t s) {
    const int S = c.n_scales, R = 2 * B;
    // the image: TimeRow[B] | per scale StftRow[2B] | f0 int64 [S][B]
    const size_t o_time = 0, o_stft = o_time + sizeof(TimeRow) * (size_t)B, o_f0 = o_stft + sizeof(StftRow) * (size_t)R * S;
    const size_t bytes = o_f0 + sizeof(int64_t) * (size_t)S * B;
    std::vector<unsigned char> img(bytes);
    TimeRow* tr = reinterpret_cast<TimeRow*>(img.data() + o_time);
    StftRow* sr_ = reinterpret_cast<StftRow*>(img.data() + o_stft);
    int64_t* f0 = reinterpret_cast<int64_t*>(img.data() + o_f0);
    int64_t n_part = 0, max_blk = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t nblk = (n[b] + kQualityBlock - 1) / kQualityBlock;
        tr[b] = TimeRow{est + est_off[b], ref + ref_off[b], n[b], n_part};
        n_part += nblk;
        max_blk = nblk > max_blk ? nblk : max_blk;
    }
    FinishArgs fa = {};
    fa.n_scales = S;
    fa.log_weight = c.log_weight;
    fa.mag_weight = c.mag_weight;
    int64_t fs_total = 0, mag_floats = 0, mel_floats = 0, max_frames[NC_QUALITY_MAX_SCALES] = {};
    for (int i = 0; i < S; ++i) {
        const int K = c.W[i] / 2 + 1;
        int64_t frames = 0;
        for (int rI = 0; rI < R; ++rI) {
            const int b = rI % B;
            const int64_t F = 1 + n[b] / c.H[i];
            StftRow& w = sr_[(size_t)i * R + rI];
            w = StftRow{rI < B ? est + est_off[b] : ref + ref_off[b], n[b], F, 0, frames * K, frames * c.n_mels[i], frames};
            if (rI < B) f0[(size_t)i * B + b] = frames;
            frames += F;
            max_frames[i] = F > max_frames[i] ? F : max_frames[i];
        }
        int64_t est_frames = 0;
        for (int b = 0; b < B; ++b) est_frames += 1 + n[b] / c.H[i];
        fa.M[i] = c.n_mels[i];
        fa.H[i] = c.H[i];
        fa.fs_off[i] = fs_total;
        fs_total += est_frames;
        mag_floats = frames * K > mag_floats ? frames * K : mag_floats;
        mel_floats = frames * c.n_mels[i] > mel_floats ? frames * c.n_mels[i] : mel_floats;
    }
    if (max_blk > (int64_t)0x7fffffff * 64) fail(NC_EINVAL, "a row is too long for one launch");
    q.call.begin(s);
    q.mag.reserve((size_t)mag_floats * sizeof(float));
    q.melbuf.reserve((size_t)mel_floats * sizeof(float));
    q.fs.reserve((size_t)fs_total * 2 * sizeof(double));
    q.part.reserve((size_t)n_part * 3 * sizeof(double));
    q.part_bad.reserve((size_t)n_part * sizeof(int32_t));
    q.state.reserve((size_t)B * kRowState * sizeof(double));
    q.row_bad.reserve((size_t)B * sizeof(int32_t));
    const float* basis[NC_QUALITY_MAX_SCALES];
    const MelDev* mels[NC_QUALITY_MAX_SCALES];
    for (int i = 0; i < S; ++i) {
        basis[i] = basis_on(q, c.W[i], NC_WINDOW_HANN);
        mels[i] = &mel_on(q, sr, c.n_mels[i], c.W[i], c.fmin[i], c.fmax[i]);
    }
    unsigned char* dev = static_cast<unsigned char*>(q.call.upload(img.data(), bytes, s));
    const TimeRow* d_tr = reinterpret_cast<const TimeRow*>(dev + o_time);
    const StftRow* d_sr = reinterpret_cast<const StftRow*>(dev + o_stft);
    const int64_t* d_f0 = reinterpret_cast<const int64_t*>(dev + o_f0);
    double* fs_mag = q.fs.as<double>();
    double* fs_log = fs_mag + fs_total;
    const dim3 tg((unsigned)((max_blk + 63) / 64), (unsigned)B), fg((unsigned)((B + 63) / 64));
    auto finish = [&](int phase) {
        hipLaunchKernelGGL(quality_finish_kernel, fg, dim3(64), 0, s, phase, d_tr, B, n_part, q.part.as<double>(), q.part_bad.as<int32_t>(), q.state.as<double>(),
                           q.row_bad.as<int32_t>(), d_f0, fs_mag, fs_log, fa, out);
    };
    hipLaunchKernelGGL(quality_time_kernel<1>, tg, dim3(64), 0, s, d_tr, q.state.as<double>(), n_part, q.part.as<double>(), q.part_bad.as<int32_t>());
    finish(1);
    hipLaunchKernelGGL(quality_time_kernel<2>, tg, dim3(64), 0, s, d_tr, q.state.as<double>(), n_part, q.part.as<double>(), q.part_bad.as<int32_t>());
    finish(2);
    hipLaunchKernelGGL(quality_time_kernel<3>, tg, dim3(64), 0, s, d_tr, q.state.as<double>(), n_part, q.part.as<double>(), q.part_bad.as<int32_t>());
    for (int i = 0; i < S; ++i) {
        const StftRow* rows = d_sr + (size_t)i * R;
        launch_stft(rows, R, max_frames[i], basis[i], c.W[i], c.H[i], nullptr, q.mag.as<float>(), s);
        launch_mel(rows, R, max_frames[i], q.mag.as<float>(), *mels[i], c.W[i] / 2 + 1, c.n_mels[i], q.melbuf.as<float>(), s);
        hipLaunchKernelGGL(mel_frame_sums_kernel, dim3((unsigned)((max_frames[i] + 255) / 256), (unsigned)B), dim3(256), 0, s, rows, B, q.melbuf.as<float>(),
                           c.n_mels[i], c.clamp_eps, fs_mag + fa.fs_off[i], fs_log + fa.fs_off[i]);
    }
    finish(3);
    q.call.end(s);
}

// STFT and / or mel spectrogram of B rows of one buffer
void run_spectra(QualityDev& q, const float* pcm, int B, const int64_t* off, const int64_t* n, int W, int H, int window, float* out_c64,
                 const MelDev* md, int M, float* out_mel, const int64_t* out_off, hipStream_t s) {
    const int K = W / 2 + 1;
    std::vector<StftRow> rows((size_t)B);
    int64_t frames = 0, max_frames = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t F = 1 + n[b] / H;
        rows[(size_t)b] = StftRow{pcm + off[b], n[b], F, out_off[b], frames * K, out_off[b], frames};
        frames += F;
        max_frames = F > max_frames ? F : max_frames;
    }
    q.call.begin(s);
    if (md) q.mag.reserve((size_t)frames * K * sizeof(float));
    const float* basis = basis_on(q, W, window);
    const StftRow* d_rows = q.call.upload(rows, s);
    launch_stft(d_rows, B, max_frames, basis, W, H, out_c64, md ? q.mag.as<float>() : nullptr, s);
    if (md) launch_mel(d_rows, B, max_frames, q.mag.as<float>(), *md, K, M, out_mel, s);
    q.call.end(s);
}

}  // namespace

}  // namespace nc

using namespace nc;

extern "C" nc_status nc_audio_stft_dev(int device_index, const float* pcm, int32_t B, const int64_t* off, const int64_t* n, int32_t W, int32_t H,
                                       int32_t window, float* out_c64, const int64_t* out_off, void* hip_stream) {
    return guard([&] {
        if (!pcm || !out_c64) fail(NC_EINVAL, "null pointer");
        quality_check_window(W, H, window);
        const int64_t* offs[2] = {off, out_off};
        quality_check_rows(B, offs, 2, n, &W, 1);
        g_quality.locked(device_index, [&](QualityDev& q) {
            run_spectra(q, pcm, B, off, n, W, H, window, out_c64, nullptr, 0, nullptr, out_off, static_cast<hipStream_t>(hip_stream));
        });
    });
}

extern "C" nc_status nc_audio_mel_spectrogram_dev(int device_index, const float* pcm, int32_t B, const int64_t* off, const int64_t* n,
                                                  int32_t sample_rate, int32_t W, int32_t H, int32_t n_mels, float fmin, float fmax, float* out,
                                                  const int64_t* out_off, void* hip_stream) {
    return guard([&] {
        if (!pcm || !out) fail(NC_EINVAL, "null pointer");
        quality_check_window(W, H, NC_WINDOW_HANN);
        if (fmax == 0.0f && sample_rate > 0) fmax = (float)sample_rate / 2.0f;
        quality_check_mel(sample_rate, n_mels, fmin, fmax);
        const int64_t* offs[2] = {off, out_off};
        quality_check_rows(B, offs, 2, n, &W, 1);
        g_quality.locked(device_index, [&](QualityDev& q) {
            const MelDev& md = mel_on(q, sample_rate, n_mels, W, fmin, fmax);
            run_spectra(q, pcm, B, off, n, W, H, NC_WINDOW_HANN, nullptr, &md, n_mels, out, out_off, static_cast<hipStream_t>(hip_stream));
        });
    });
}

extern "C" nc_status nc_quality_metrics_dev(int device_index, const float* ref, const int64_t* ref_off, const float* est, const int64_t* est_off,
                                            const int64_t* n, int32_t B, int32_t sample_rate, const nc_quality_cfg* cfg, nc_quality_row* out,
                                            void* hip_stream) {
    return guard([&] {
        if (!ref || !est || !out) fail(NC_EINVAL, "null pointer");
        const nc_quality_cfg c = quality_resolve_cfg(cfg, sample_rate);
        const int64_t* offs[2] = {ref_off, est_off};
        quality_check_rows(B, offs, 2, n, c.W, c.n_scales);
        g_quality.locked(device_index, [&](QualityDev& q) {
            run_metrics(q, ref, ref_off, est, est_off, n, B, sample_rate, c, out, static_cast<hipStream_t>(hip_stream));
        });
    });
}

extern "C" nc_status nc_quality_metrics(int device_index, const float* ref, const int64_t* ref_off, const float* est, const int64_t* est_off,
                                        const int64_t* n, int32_t B, int32_t sample_rate, const nc_quality_cfg* cfg, nc_quality_row* out) {
    return guard([&] {
        if (!ref || !est || !out) fail(NC_EINVAL, "null pointer");
        const nc_quality_cfg c = quality_resolve_cfg(cfg, sample_rate);
        const int64_t* offs[2] = {ref_off, est_off};
        quality_check_rows(B, offs, 2, n, c.W, c.n_scales);
        g_quality.locked(device_index, [&](QualityDev& q) {
            const PackedRows packed(B, n, 1, 1);   // HOST rows end to end, no padding
            packed.copy_in(q.in_est, est, est_off);
            packed.copy_in(q.in_ref, ref, ref_off);
            q.out_rows.reserve((size_t)B * sizeof(nc_quality_row));
            run_metrics(q, q.in_ref.as<float>(), packed.at.data(), q.in_est.as<float>(), packed.at.data(), n, B, sample_rate, c, q.out_rows.as<nc_quality_row>(),
                        nullptr);
            NC_HIP(hipStreamSynchronize(nullptr));
            NC_HIP(hipMemcpy(out, q.out_rows.p, (size_t)B * sizeof(nc_quality_row), hipMemcpyDeviceToHost));
        });
    });
}
