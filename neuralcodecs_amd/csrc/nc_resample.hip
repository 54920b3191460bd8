// Band-limited resampling on the device (include/nc_mi355x.h "band-limited resampling").  The arithmetic of every output
// sample is the one chain the header states, so the results equal the serial host twin (nc_resample_host.hip) bit for bit; the two units
// share nc_math.h, the host table builder and the argument checks (nc_resample.h) and nothing else.
//
// resample_mfma_kernel: y[m U + i] = sum_k h[i][k] xpad[m D + k] as D[16 phases][16 frames] = A B with v_mfma_f32_16x16x4_f32, whose result
// is the k-ordered fmaf chain.  A workgroup (4 waves) serves 16 consecutive frames of one row: it stages the stretch of 15 D + K4 padded
// samples once (the edge sample repeated, resolved while staging), sample i at word i + s (i / D) with s chosen so that the frame stride
// D + s is 2 (mod 4): the 16 frames of one tap (lanes 0..15) then fall into 16 distinct even banks of the 32 a ds_read_b32 half-wave sees
// and the tap beside it (lanes 16..31) into the odd ones.  The waves take the phase tiles in turn, one accumulator each: no chain is split.
// The A operand comes straight from the cached table image, stored per row as four runs [k % 4][k / 4] (each run padded to a multiple of
// four words) so that a lane's taps of four consecutive instructions are one 16-byte load.  A lane's four results are four consecutive
// phases of one frame, i.e. four consecutive output samples: one 16-byte store where the address allows it.
// resample_vec_kernel: the same chain, one thread per output sample, straight from global memory -- for ratios whose U leaves a 16-phase
// tile mostly empty (U < 8) or whose stretch does not fit the LDS budget of one workgroup.
#include <tuple>

#include "nc_devcall.h"
#include "nc_frag.h"
#include "nc_guard.h"
#include "nc_math.h"
#include "nc_resample.h"

namespace nc {

namespace {

constexpr int kFrames = 16;                    // frames per workgroup: the columns of one matrix-core tile
constexpr int kMfmaMinU = 8;                   // below: a phase tile is more than half empty
constexpr size_t kLdsBudget = 64 * 1024;       // bytes of one workgroup's stretch (the default limit of dynamic LDS)

struct RsRow {
    const float* x;
    float* y;
    int64_t n, n_out;
};

struct RsArgs {
    int U, D, W, K4;
    int Q4;          // words per run of the table image
    int skew;        // s: extra words per D staged samples
    int tiles;       // phase tiles: ceil(U / 16)
};

__global__ __launch_bounds__(256) void resample_mfma_kernel(const RsRow* __restrict__ rows, const float* __restrict__ T, RsArgs g) {
    extern __shared__ float xs[];
    const RsRow r = rows[blockIdx.y];
    const int64_t frames = (r.n_out + g.U - 1) / g.U;
    const int64_t m0 = (int64_t)blockIdx.x * kFrames;
    if (m0 >= frames) return;   // the whole workgroup: before any barrier
    const int S = (kFrames - 1) * g.D + g.K4;
    const int64_t j0 = m0 * g.D - g.W, last = r.n - 1;
    for (int i = threadIdx.x; i < S; i += 256) {
        int64_t j = j0 + i;
        j = j < 0 ? 0 : (j > last ? last : j);
        xs[i + (g.skew ? g.skew * (i / g.D) : 0)] = r.x[j];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rr = lane & 15, kq = lane >> 4;
    const int J = g.K4 >> 2;
    const float* xb = xs + rr * (g.D + g.skew) + kq;
    const int64_t m = m0 + rr;
    for (int pt = wave; pt < g.tiles; pt += 4) {
        const float* ap = T + ((size_t)(16 * pt + rr) * 4 + (size_t)kq) * (size_t)g.Q4;
        f32x4_t acc = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};
        int rem = kq, sk = 0;   // tap t = 4 j + kq of this lane: rem = t mod D, sk = s (t / D); kept only where skew != 0 (then D >= 4)
        for (int j4 = 0; j4 < J; j4 += 4) {
            const f32x4_t a = *reinterpret_cast<const f32x4_t*>(ap + j4);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (j4 + u < J) {   // the same for every lane
                    const float b = xb[4 * (j4 + u) + sk];
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b, acc, 0, 0, 0);
                    if (g.skew) {
                        rem += 4;
                        const bool wrap = rem >= g.D;
                        rem -= wrap ? g.D : 0;
                        sk += wrap ? g.skew : 0;
                    }
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = acc[e] != acc[e] ? __builtin_bit_cast(float, 0x7fc00000u) : acc[e];
        const int p = 16 * pt + 4 * kq;
        const int64_t o = m * g.U + p;
        if (p >= g.U || o >= r.n_out) continue;
        float* dst = r.y + o;
        if (p + 4 <= g.U && o + 4 <= r.n_out && ((uintptr_t)dst & 15u) == 0) {
            *reinterpret_cast<f32x4_t*>(dst) = acc;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (p + e < g.U && o + e < r.n_out) dst[e] = acc[e];
        }
    }
}

__global__ __launch_bounds__(256) void resample_vec_kernel(const RsRow* __restrict__ rows, const float* __restrict__ T, RsArgs g) {
    const RsRow r = rows[blockIdx.y];
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= r.n_out) return;
    const int64_t m = o / g.U;
    const int i = (int)(o - m * g.U);
    const float* hi = T + (size_t)i * 4 * (size_t)g.Q4;
    const int64_t j0 = m * g.D - g.W, last = r.n - 1;
    float acc = 0.0f;
    for (int q = 0; q < (g.K4 >> 2); ++q) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int64_t j = j0 + 4 * q + e;
            j = j < 0 ? 0 : (j > last ? last : j);
            acc = nc_fma(hi[(size_t)e * g.Q4 + q], r.x[j], acc);
        }
    }
    r.y[o] = acc != acc ? __builtin_bit_cast(float, 0x7fc00000u) : acc;
}

// src == dst
__global__ __launch_bounds__(256) void resample_copy_kernel(const RsRow* __restrict__ rows) {
    const RsRow r = rows[blockIdx.y];
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o < r.n_out) r.y[o] = r.x[o];
}

// ---- per-device state: the cached table images beside the call scaffold (nc_devcall.h) -------------------------------------------------
struct RsDev {
    DevCall call;
    std::map<std::tuple<int64_t, int64_t, int, uint64_t>, DevBuf> tabs;   // (U, D, zeros, the bits of rolloff)
    DevBuf in, out;
};

PerDevice<RsDev> g_resample;

RsArgs args_of(const ResampleGeom& q) {
    RsArgs a;
    a.U = (int)q.U;
    a.D = (int)q.D;
    a.W = (int)q.W;
    a.K4 = (int)q.K4;
    a.Q4 = (int)(((q.K4 >> 2) + 3) & ~(int64_t)3);
    a.skew = q.D < 4 ? 0 : (int)((6 - q.D % 4) % 4);
    a.tiles = (int)((q.U + 15) / 16);
    return a;
}

// words of the staged stretch, skew included
int64_t lds_words(const ResampleGeom& q, const RsArgs& a) {
    const int64_t S = (kFrames - 1) * q.D + q.K4;
    return S + (int64_t)a.skew * ((S - 1) / q.D) + 1;
}

bool takes_mfma(const ResampleGeom& q, const RsArgs& a) { return q.U >= kMfmaMinU && (size_t)lds_words(q, a) * sizeof(float) <= kLdsBudget; }

const float* table_on(RsDev& d, const ResampleGeom& q, const RsArgs& a) {
    return cached_table(d.tabs[std::make_tuple(q.U, q.D, q.zeros, __builtin_bit_cast(uint64_t, q.rolloff))], [&](DevBuf& t) {
        std::vector<float> h;
        build_resample_table(q, h);
        const size_t row = (size_t)4 * a.Q4;
        std::vector<float> img((size_t)16 * a.tiles * row, 0.0f);   // rows U .. 16 tiles - 1 and the tail of every run stay +0
        for (int64_t i = 0; i < q.U; ++i)
            for (int64_t k = 0; k < q.K4; ++k) img[(size_t)i * row + (size_t)(k & 3) * a.Q4 + (size_t)(k >> 2)] = h[(size_t)(i * q.K4 + k)];
        fill_table(t, img.data(), img.size());
    }).as<float>();
}

unsigned grid_of(int64_t items, int per_block) { return nc::grid_of(items, per_block, 0xffffff); }   // 256 threads each: below 2^32 in all

void run_resample(RsDev& d, const ResampleGeom& q, bool copy, const float* pcm, int R, const int64_t* off, const int64_t* n, float* out,
                  const int64_t* out_off, hipStream_t s) {
    std::vector<RsRow> rows((size_t)R);
    int64_t max_out = 0;
    for (int r = 0; r < R; ++r) {
        const int64_t no = copy ? n[r] : resample_len(n[r], q.U, q.D);
        rows[(size_t)r] = RsRow{pcm + off[r], out + out_off[r], n[r], no};
        max_out = no > max_out ? no : max_out;
    }
    if (max_out == 0) return;
    const RsArgs a = args_of(q);
    const bool mfma = !copy && takes_mfma(q, a);
    const unsigned gx = mfma ? grid_of((max_out + q.U - 1) / q.U, kFrames) : grid_of(max_out, 256);
    d.call.begin(s);
    const float* T = copy ? nullptr : table_on(d, q, a);
    const RsRow* d_rows = d.call.upload(rows, s);
    if (copy)
        hipLaunchKernelGGL(resample_copy_kernel, dim3(gx, (unsigned)R), dim3(256), 0, s, d_rows);
    else if (mfma)
        hipLaunchKernelGGL(resample_mfma_kernel, dim3(gx, (unsigned)R), dim3(256), (size_t)lds_words(q, a) * sizeof(float), s, d_rows, T, a);
    else
        hipLaunchKernelGGL(resample_vec_kernel, dim3(gx, (unsigned)R), dim3(256), 0, s, d_rows, T, a);
    d.call.end(s);
}

}  // namespace

}  // namespace nc

using namespace nc;

extern "C" nc_status nc_audio_resample_sinc_dev(int device_index, const float* pcm, int32_t R, const int64_t* off, const int64_t* n, int32_t src,
                                                int32_t dst, const nc_resample_cfg* cfg, float* out, const int64_t* out_off, void* hip_stream) {
    return guard([&] {
        const ResampleGeom q = resample_geom(src, dst, cfg);
        resample_check_rows(pcm, R, off, n, q, src == dst, out, out_off);
        g_resample.locked(device_index, [&](RsDev& d) {
            run_resample(d, q, src == dst, pcm, R, off, n, out, out_off, static_cast<hipStream_t>(hip_stream));
        });
    });
}

extern "C" nc_status nc_audio_resample_sinc(int device_index, const float* pcm, int32_t R, const int64_t* off, const int64_t* n, int32_t src,
                                            int32_t dst, const nc_resample_cfg* cfg, float* out, const int64_t* out_off) {
    return guard([&] {
        const ResampleGeom q = resample_geom(src, dst, cfg);
        const bool copy = src == dst;
        resample_check_rows(pcm, R, off, n, q, copy, out, out_off);
        g_resample.locked(device_index, [&](RsDev& d) {
            // HOST rows -> the device staging buffers, every row at a multiple of four elements (the 16-byte store of the matrix-core kernel)
            std::vector<int64_t> no((size_t)R);
            for (int r = 0; r < R; ++r) no[(size_t)r] = copy ? n[r] : resample_len(n[r], q.U, q.D);
            const PackedRows pin(R, n, 1, 4), pout(R, no.data(), 1, 4);
            pin.copy_in(d.in, pcm, off);
            pout.reserve(d.out);
            run_resample(d, q, copy, d.in.as<float>(), R, pin.at.data(), n, d.out.as<float>(), pout.at.data(), nullptr);
            NC_HIP(hipStreamSynchronize(nullptr));
            pout.copy_out(d.out, out, out_off);
        });
    });
}
