// Loudness on the device (include/nc_mi355x.h "loudness"): the K-weighting recursion in block-parallel form on the fp32
// matrix cores, the serial state scan, the energies, both gates and the gain.  The arithmetic of every output element is the one chain the
// header states, so the results equal the serial host twin (nc_loudness_host.hip) bit for bit; the two units share nc_math.h, the host
// table builder and the argument checks (nc_loudness.h) and nothing else.
//
// kweight_mfma_kernel: D[80][columns] = [Hm; Cm; 12 zero rows] X with v_mfma_f32_16x16x4_f32, whose result is the k-ordered fmaf chain; a
// column is one 64-sample block of one row.  A workgroup (4 waves) serves 64 consecutive blocks of a row: it stages that stretch of 4096
// samples once (zero past the row end), sample i at word i + 2 (i / 64), so the 16 columns of one tap fall into 16 distinct even banks
// and the tap beside it (lanes +16) into the odd ones.  A wave holds five accumulators (rows 0..79) over ONE B operand of 16 columns; no
// chain is split.  The A operand comes straight from the cached 20 KB table, stored per row as four runs [k % 4][k / 4] so that a lane's
// taps of four consecutive instructions are one 16-byte load.  u goes out as [column][64], v as [column][4].
// kweight_scan_kernel: one thread per row, serial over its blocks in binary64: s_q of every block.
// kweight_out_kernel: y = fl(u + Gs[r] . s_q), one thread per sample (in place over u for the loudness calls).
// loud_*_kernel: sub-block sums, cell sums, block sums and the per-clip finish, each in the stated order; no floating-point atomics (the
// count of non-finite samples is an integer atomic).
#include "nc_devcall.h"
#include "nc_frag.h"
#include "nc_guard.h"
#include "nc_loudness.h"
#include "nc_math.h"

namespace nc {

namespace {

constexpr int kColsPerBlock = 64, kColStride = kKwBlock + 2, kTableRows = 80;

struct KwRow {
    const float* x;
    float* y;           // where the filtered row goes (the gain kernel: where the scaled row goes)
    int64_t n;
    int64_t col0;       // first block of this row among the columns of the call
    int64_t J;          // gating blocks of the clip
    int64_t p0, c0, z0; // first sub-block sum, cell sum and block energy of this row
    int64_t w0;         // first W_j of the clip
    int32_t clip, pad;
};

__global__ __launch_bounds__(256) void kweight_mfma_kernel(const KwRow* __restrict__ rows, const float* __restrict__ T, float* __restrict__ U,
                                                           float* __restrict__ V, unsigned long long* __restrict__ bad) {
    __shared__ float xs[kColsPerBlock * kColStride];
    const KwRow r = rows[blockIdx.y];
    const int64_t nblk = (r.n + kKwBlock - 1) / kKwBlock;
    const int64_t q0 = (int64_t)blockIdx.x * kColsPerBlock;
    if (q0 >= nblk) return;   // the whole workgroup: before any barrier
    const int64_t s0 = q0 * kKwBlock;
    int nbad = 0;
    for (int i = threadIdx.x; i < kColsPerBlock * kKwBlock; i += 256) {
        const int64_t p = s0 + i;
        float v = 0.0f;
        if (p < r.n) {
            v = r.x[p];
            nbad += finite32(v) ? 0 : 1;
        }
        xs[i + 2 * (i >> 6)] = v;
    }
    if (bad != nullptr && nbad != 0) atomicAdd(&bad[r.clip], (unsigned long long)nbad);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rr = lane & 15, kq = lane >> 4;
    const int c = wave * 16 + rr;
    const float* ap[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) ap[i] = T + (size_t)(16 * i + rr) * kKwBlock + (size_t)kq * 16;
    const float* xb = xs + c * kColStride + kq;
    f32x4_t acc[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) acc[i] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int u4 = 0; u4 < 16; u4 += 4) {
        f32x4_t a[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) a[i] = *reinterpret_cast<const f32x4_t*>(ap[i] + u4);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float b = xb[4 * (u4 + u)];
#pragma unroll
            for (int i = 0; i < 5; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][u], b, acc[i], 0, 0, 0);
        }
    }
    const int64_t q = q0 + c;
    if (q >= nblk) return;
    const int64_t col = r.col0 + q;
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4_t*>(U + col * kKwBlock + 16 * i + 4 * kq) = acc[i];
    if (kq == 0) *reinterpret_cast<f32x4_t*>(V + col * 4) = acc[4];
}

__device__ __forceinline__ double dot_state(const double* w, const double* s) { return ((w[0] * s[0] + w[1] * s[1]) + w[2] * s[2]) + w[3] * s[3]; }

__global__ __launch_bounds__(64) void kweight_scan_kernel(const KwRow* __restrict__ rows, int R, const double* __restrict__ M, const float* __restrict__ V,
                                                          double* __restrict__ Sq) {
    const int ri = blockIdx.x * 64 + threadIdx.x;
    if (ri >= R) return;
    const KwRow r = rows[ri];
    const int64_t nblk = (r.n + kKwBlock - 1) / kKwBlock;
    double m[4][4], s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) m[i][k] = M[4 * i + k];
    for (int64_t q = 0; q < nblk; ++q) {
        const int64_t col = r.col0 + q;
        const f32x4_t v = *reinterpret_cast<const f32x4_t*>(V + col * 4);
        double s1[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            Sq[col * 4 + i] = s[i];
            s1[i] = dot_state(m[i], s) + (double)v[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = s1[i];
    }
}

__global__ __launch_bounds__(256) void kweight_out_kernel(const KwRow* __restrict__ rows, const double* __restrict__ Gs, const float* U,
                                                          const double* __restrict__ Sq) {
    const KwRow r = rows[blockIdx.y];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= r.n) return;
    const int64_t col = r.col0 + (i >> 6);
    const int rI = (int)(i & 63);
    double s[4], g[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        s[k] = Sq[col * 4 + k];
        g[k] = Gs[4 * rI + k];
    }
    const float u = U[col * kKwBlock + rI];
    r.y[i] = (float)((double)u + dot_state(g, s));   // (the loudness calls: r.y + i is the word u came from)
}

// one thread per sub-block of a cell: the samples ascending
__global__ __launch_bounds__(64) void loud_sub_kernel(const KwRow* __restrict__ rows, int S, int nsub, double* __restrict__ part) {
    const KwRow r = rows[blockIdx.y];
    const int64_t items = r.J > 0 ? (r.J + 3) * nsub : 0;
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= items) return;
    const int64_t cell = t / nsub;
    const int k0 = (int)(t % nsub) * kLoudSub;
    const int k1 = k0 + kLoudSub < S ? k0 + kLoudSub : S;
    const float* y = r.y + cell * S;
    double sub = 0.0;
    for (int k = k0; k < k1; ++k) {
        const float v = y[k];
        sub = sub + (double)(v * v);
    }
    part[r.p0 + t] = sub;
}

// one thread per cell: its sub-blocks ascending
__global__ __launch_bounds__(64) void loud_cell_kernel(const KwRow* __restrict__ rows, int nsub, const double* __restrict__ part, double* __restrict__ cells) {
    const KwRow r = rows[blockIdx.y];
    const int64_t ncell = r.J > 0 ? r.J + 3 : 0;
    const int64_t cell = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (cell >= ncell) return;
    const double* p = part + r.p0 + cell * nsub;
    double acc = 0.0;
    for (int k = 0; k < nsub; ++k) acc = acc + p[k];
    cells[r.c0 + cell] = acc;
}

// one thread per gating block: four cells, then the remainder of the block sample by sample
__global__ __launch_bounds__(64) void loud_block_kernel(const KwRow* __restrict__ rows, int N, int S, const double* __restrict__ cells, double* __restrict__ z) {
    const KwRow r = rows[blockIdx.y];
    const int64_t j = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (j >= r.J) return;
    const double* cl = cells + r.c0 + j;
    double sum = ((cl[0] + cl[1]) + cl[2]) + cl[3];
    for (int64_t k = (j + 4) * S; k < j * S + N; ++k) {
        const float v = r.y[k];
        sum = sum + (double)(v * v);
    }
    z[r.z0 + j] = sum / (double)N;
}

__device__ __forceinline__ float channel_gain(int c) { return c < 3 ? 1.0f : 1.41f; }

// one thread per clip: W_j, both gates, the means and the formulas
__global__ __launch_bounds__(64) void loud_finish_kernel(const KwRow* __restrict__ rows, int B, int C, const double* __restrict__ z, double* __restrict__ W,
                                                         const unsigned long long* __restrict__ bad, float target_db, nc_loudness_row* __restrict__ out) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const KwRow* cr = rows + (size_t)b * C;
    const int64_t J = cr[0].J;
    nc_loudness_row o = {};
    o.n_blocks = (int32_t)(J > 0x7fffffff ? 0x7fffffff : J);
    const unsigned long long nb = bad[b];
    o.n_bad = (int32_t)(nb > 0x7fffffffull ? 0x7fffffffull : nb);
    if (nb != 0) {
        o.lufs = o.gain = __builtin_nanf("");
        out[b] = o;
        return;
    }
    double* Wc = W + cr[0].w0;
    int64_t na = 0, nr = 0;
    for (int64_t j = 0; j < J; ++j) {
        double w = 0.0;
        for (int c = 0; c < C; ++c) w = w + (double)channel_gain(c) * z[cr[c].z0 + j];
        Wc[j] = w;
        na += w > kGateAbs ? 1 : 0;
    }
    double Wa = 0.0, Wr = 0.0;
    for (int c = 0; c < C; ++c) {
        const double* zc = z + cr[c].z0;
        double acc = 0.0;
        for (int64_t j = 0; j < J; ++j)
            if (Wc[j] > kGateAbs) acc = acc + zc[j];
        Wa = Wa + (double)channel_gain(c) * (acc / (double)(na > 1 ? na : 1));
    }
    const double rel = 0.1 * Wa;
    for (int64_t j = 0; j < J; ++j) nr += (Wc[j] > kGateAbs && Wc[j] > rel) ? 1 : 0;
    for (int c = 0; c < C; ++c) {
        const double* zc = z + cr[c].z0;
        double acc = 0.0;
        for (int64_t j = 0; j < J; ++j)
            if (Wc[j] > kGateAbs && Wc[j] > rel) acc = acc + zc[j];
        Wr = Wr + (double)channel_gain(c) * (acc / (double)(nr > 1 ? nr : 1));
    }
    o.n_pass_abs = (int32_t)(na > 0x7fffffff ? 0x7fffffff : na);
    o.n_pass_rel = (int32_t)(nr > 0x7fffffff ? 0x7fffffff : nr);
    const float wf = (float)Wr;
    float lufs = -70.0f;
    if (wf >= 1.17549435e-38f) {
        const float l = -0.691f + 10.0f * nc_log10f(wf);
        lufs = l > -70.0f ? l : -70.0f;
    }
    o.lufs = lufs;
    o.gain = nc_expf((target_db - lufs) * kGainFactor);
    out[b] = o;
}

// y = fl(x gain): four samples per thread, one 16-byte load and store where both rows are 16-byte aligned, scalar otherwise and at the tail
__global__ __launch_bounds__(256) void gain_kernel(const KwRow* __restrict__ rows, const float* __restrict__ gains, int stride) {
    const KwRow r = rows[blockIdx.y];
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= r.n) return;
    const float g = gains[(size_t)r.clip * stride];
    const bool is_nan = g != g;
    const float qnan = __builtin_bit_cast(float, 0x7fc00000u);
    const bool aligned = (((uintptr_t)r.x | (uintptr_t)r.y) & 15u) == 0;
    if (aligned && i0 + 4 <= r.n) {
        const f32x4_t v = *reinterpret_cast<const f32x4_t*>(r.x + i0);
        f32x4_t o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = is_nan ? qnan : v[k] * g;
        *reinterpret_cast<f32x4_t*>(r.y + i0) = o;
        return;
    }
    for (int k = 0; k < 4 && i0 + k < r.n; ++k) {
        const float v = r.x[i0 + k];
        r.y[i0 + k] = is_nan ? qnan : v * g;
    }
}

// ---- per-device state: the cached tables and one workspace beside the call scaffold (nc_devcall.h) --------------------------------------
struct KwDev {
    DevBuf T, Gs, M;
};
bool filled(const KwDev& d) { return d.T.p != nullptr; }

struct LoudDev {
    DevCall call;
    std::map<std::pair<int, int>, KwDev> tabs;   // (rate or 0, filter)
    DevBuf U, V, Sq, part, cells, z, W, bad, in, out, out_rows;
};

PerDevice<LoudDev> g_loud;

const KwDev& tables_on(LoudDev& q, int sample_rate, int filter) {
    return cached_table(q.tabs[{filter == NC_KWEIGHT_REFERENCE ? 0 : sample_rate, filter}], [&](KwDev& d) {
        KwTables t;
        build_kweight_tables(sample_rate, filter, t);
        std::vector<float> T((size_t)kTableRows * kKwBlock, 0.0f);
        for (int row = 0; row < kKwBlock + 4; ++row)
            for (int k = 0; k < kKwBlock; ++k)
                T[(size_t)row * kKwBlock + (size_t)(k & 3) * 16 + (size_t)(k >> 2)] = row < kKwBlock ? t.Hm[(size_t)row * kKwBlock + k] : t.Cm[(size_t)(row - kKwBlock) * kKwBlock + k];
        fill_table(d.Gs, &t.Gs[0][0], sizeof(t.Gs) / sizeof(double));
        fill_table(d.M, &t.M[0][0], sizeof(t.M) / sizeof(double));
        fill_table(d.T, T.data(), T.size());
    });
}

unsigned grid_of(int64_t items, int per_block) { return nc::grid_of(items, per_block, 0x7fffffff); }

// GEMM, scan and output of the rows d_rows[0..R) (their y set); the workspace U / V / Sq is reserved by the caller
void launch_filter(LoudDev& q, const KwDev& kd, const KwRow* d_rows, int R, int64_t max_n, unsigned long long* bad, hipStream_t s) {
    if (max_n <= 0) return;
    const int64_t max_blk = (max_n + kKwBlock - 1) / kKwBlock;
    hipLaunchKernelGGL(kweight_mfma_kernel, dim3(grid_of(max_blk, kColsPerBlock), (unsigned)R), dim3(256), 0, s, d_rows, kd.T.as<float>(), q.U.as<float>(),
                       q.V.as<float>(), bad);
    hipLaunchKernelGGL(kweight_scan_kernel, dim3((unsigned)((R + 63) / 64)), dim3(64), 0, s, d_rows, R, kd.M.as<double>(), q.V.as<float>(), q.Sq.as<double>());
    hipLaunchKernelGGL(kweight_out_kernel, dim3(grid_of(max_n, 256), (unsigned)R), dim3(256), 0, s, d_rows, kd.Gs.as<double>(), q.U.as<float>(), q.Sq.as<double>());
}

void reserve_filter(LoudDev& q, int64_t cols) {
    q.U.reserve((size_t)cols * kKwBlock * sizeof(float));
    q.V.reserve((size_t)cols * 4 * sizeof(float));
    q.Sq.reserve((size_t)cols * 4 * sizeof(double));
}

void run_kweight(LoudDev& q, const float* pcm, int R, const int64_t* off, const int64_t* n, int sample_rate, int filter, float* out, const int64_t* out_off,
                 hipStream_t s) {
    std::vector<KwRow> rows((size_t)R);
    int64_t cols = 0, max_n = 0;
    for (int r = 0; r < R; ++r) {
        rows[(size_t)r] = KwRow{pcm + off[r], out + out_off[r], n[r], cols, 0, 0, 0, 0, 0, 0, 0};
        cols += (n[r] + kKwBlock - 1) / kKwBlock;
        max_n = n[r] > max_n ? n[r] : max_n;
    }
    q.call.begin(s);
    reserve_filter(q, cols);
    const KwDev& kd = tables_on(q, sample_rate, filter);
    const KwRow* d_rows = q.call.upload(rows, s);
    launch_filter(q, kd, d_rows, R, max_n, nullptr, s);
    q.call.end(s);
}

// measure B clips into out_rows (device); with `out`, also write the levelled clips
void run_loudness(LoudDev& q, const float* pcm, int B, int C, const int64_t* off, const int64_t* n, int sample_rate, const nc_loudness_cfg& c, float* out,
                  const int64_t* out_off, nc_loudness_row* out_rows, hipStream_t s) {
    const int R = B * C;
    const LoudGeom g = loudness_geom(sample_rate);
    const int nsub = (g.S + kLoudSub - 1) / kLoudSub;
    std::vector<KwRow> rows((size_t)R * (out ? 2 : 1));
    int64_t cols = 0, max_n = 0, n_part = 0, n_cell = 0, n_z = 0, n_w = 0, max_J = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t J = n[b] >= g.N ? (n[b] - g.N) / g.S + 1 : 0;
        const int64_t ncell = J > 0 ? J + 3 : 0;
        for (int ch = 0; ch < C; ++ch) {
            const size_t r = (size_t)b * C + ch;
            rows[r] = KwRow{pcm + off[r], nullptr, n[b], cols, J, n_part, n_cell, n_z, n_w, b, 0};
            if (out) {
                rows[(size_t)R + r] = rows[r];
                rows[(size_t)R + r].y = out + out_off[r];
            }
            cols += (n[b] + kKwBlock - 1) / kKwBlock;
            n_part += ncell * nsub;
            n_cell += ncell;
            n_z += J;
        }
        n_w += J;
        max_n = n[b] > max_n ? n[b] : max_n;
        max_J = J > max_J ? J : max_J;
    }
    q.call.begin(s);
    reserve_filter(q, cols);
    q.part.reserve((size_t)n_part * sizeof(double));
    q.cells.reserve((size_t)n_cell * sizeof(double));
    q.z.reserve((size_t)n_z * sizeof(double));
    q.W.reserve((size_t)n_w * sizeof(double));
    q.bad.reserve((size_t)B * sizeof(unsigned long long));
    for (int r = 0; r < R; ++r) rows[(size_t)r].y = q.U.as<float>() + rows[(size_t)r].col0 * kKwBlock;   // y takes the place of u
    const KwDev& kd = tables_on(q, sample_rate, c.filter);
    const KwRow* d_rows = q.call.upload(rows, s);
    NC_HIP(hipMemsetAsync(q.bad.p, 0, (size_t)B * sizeof(unsigned long long), s));
    launch_filter(q, kd, d_rows, R, max_n, q.bad.as<unsigned long long>(), s);
    if (max_J > 0) {
        hipLaunchKernelGGL(loud_sub_kernel, dim3(grid_of((max_J + 3) * nsub, 64), (unsigned)R), dim3(64), 0, s, d_rows, g.S, nsub, q.part.as<double>());
        hipLaunchKernelGGL(loud_cell_kernel, dim3(grid_of(max_J + 3, 64), (unsigned)R), dim3(64), 0, s, d_rows, nsub, q.part.as<double>(), q.cells.as<double>());
        hipLaunchKernelGGL(loud_block_kernel, dim3(grid_of(max_J, 64), (unsigned)R), dim3(64), 0, s, d_rows, g.N, g.S, q.cells.as<double>(), q.z.as<double>());
    }
    hipLaunchKernelGGL(loud_finish_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, d_rows, B, C, q.z.as<double>(), q.W.as<double>(),
                       q.bad.as<unsigned long long>(), c.target_db, out_rows);
    if (out && max_n > 0)
        hipLaunchKernelGGL(gain_kernel, dim3(grid_of(max_n, 1024), (unsigned)R), dim3(256), 0, s, d_rows + R, &out_rows[0].gain,
                           (int)(sizeof(nc_loudness_row) / sizeof(float)));
    q.call.end(s);
}

void run_gain(LoudDev& q, const float* pcm, int B, int C, const int64_t* off, const int64_t* n, const float* db, float* out, const int64_t* out_off,
              hipStream_t s) {
    const int R = B * C;
    // the image: KwRow[R] | float gain[B]
    const size_t o_gain = sizeof(KwRow) * (size_t)R, bytes = o_gain + sizeof(float) * (size_t)B;
    std::vector<unsigned char> img(bytes);
    KwRow* rows = reinterpret_cast<KwRow*>(img.data());
    float* gains = reinterpret_cast<float*>(img.data() + o_gain);
    int64_t max_n = 0;
    for (int b = 0; b < B; ++b) {
        gains[b] = nc_expf(db[b] * kGainFactor);
        for (int ch = 0; ch < C; ++ch) {
            const size_t r = (size_t)b * C + ch;
            rows[r] = KwRow{pcm + off[r], out + out_off[r], n[b], 0, 0, 0, 0, 0, 0, b, 0};
        }
        max_n = n[b] > max_n ? n[b] : max_n;
    }
    q.call.begin(s);
    unsigned char* dev = static_cast<unsigned char*>(q.call.upload(img.data(), bytes, s));
    if (max_n > 0)
        hipLaunchKernelGGL(gain_kernel, dim3(grid_of(max_n, 1024), (unsigned)R), dim3(256), 0, s, reinterpret_cast<const KwRow*>(dev),
                           reinterpret_cast<const float*>(dev + o_gain), 1);
    q.call.end(s);
}

void check_db(const float* db, int B) {
    if (!db) fail(NC_EINVAL, "null pointer");
    for (int b = 0; b < B; ++b)
        if (!finite32(db[b])) fail(NC_EINVAL, "db[%d] is not finite", b);
}

constexpr int64_t kStageAlign = 4;   // HOST rows lie at multiples of four elements in the staging buffers: the gain kernel's 16-byte path

// the plain calls: HOST buffers through the staging buffers, synchronous.  measure: loudness / normalize; db: apply_gain_db
void host_buffer_call(int device_index, const float* pcm, int B, int C, const int64_t* off, const int64_t* n, int sample_rate, const nc_loudness_cfg* c,
                      const float* db, float* out, const int64_t* out_off, nc_loudness_row* rows) {
    g_loud.locked(device_index, [&](LoudDev& q) {
        const PackedRows packed(B * C, n, C, kStageAlign);
        packed.copy_in(q.in, pcm, off);
        if (out) packed.reserve(q.out);
        if (c) {
            q.out_rows.reserve((size_t)B * sizeof(nc_loudness_row));
            run_loudness(q, q.in.as<float>(), B, C, packed.at.data(), n, sample_rate, *c, out ? q.out.as<float>() : nullptr, out ? packed.at.data() : nullptr,
                         q.out_rows.as<nc_loudness_row>(), nullptr);
        } else {
            run_gain(q, q.in.as<float>(), B, C, packed.at.data(), n, db, q.out.as<float>(), packed.at.data(), nullptr);
        }
        NC_HIP(hipStreamSynchronize(nullptr));
        if (c) NC_HIP(hipMemcpy(rows, q.out_rows.p, (size_t)B * sizeof(nc_loudness_row), hipMemcpyDeviceToHost));
        if (out) packed.copy_out(q.out, out, out_off);
    });
}

}  // namespace

}  // namespace nc

using namespace nc;

extern "C" nc_status nc_audio_kweight_dev(int device_index, const float* pcm, int32_t R, const int64_t* off, const int64_t* n, int32_t sample_rate,
                                          int32_t filter, float* out, const int64_t* out_off, void* hip_stream) {
    return guard([&] {
        if (!pcm || !out) fail(NC_EINVAL, "null pointer");
        loudness_check_filter(sample_rate, filter);
        const int64_t* offs[2] = {off, out_off};
        loudness_check_rows(R, offs, 2, 1, n);
        g_loud.locked(device_index, [&](LoudDev& q) { run_kweight(q, pcm, R, off, n, sample_rate, filter, out, out_off, static_cast<hipStream_t>(hip_stream)); });
    });
}

extern "C" nc_status nc_audio_kweight(int device_index, const float* pcm, int32_t R, const int64_t* off, const int64_t* n, int32_t sample_rate,
                                      int32_t filter, float* out, const int64_t* out_off) {
    return guard([&] {
        if (!pcm || !out) fail(NC_EINVAL, "null pointer");
        loudness_check_filter(sample_rate, filter);
        const int64_t* offs[2] = {off, out_off};
        loudness_check_rows(R, offs, 2, 1, n);
        g_loud.locked(device_index, [&](LoudDev& q) {
            const PackedRows packed(R, n, 1, kStageAlign);
            packed.copy_in(q.in, pcm, off);
            packed.reserve(q.out);
            run_kweight(q, q.in.as<float>(), R, packed.at.data(), n, sample_rate, filter, q.out.as<float>(), packed.at.data(), nullptr);
            NC_HIP(hipStreamSynchronize(nullptr));
            packed.copy_out(q.out, out, out_off);
        });
    });
}

extern "C" nc_status nc_loudness_dev(int device_index, const float* pcm, int32_t B, int32_t C, const int64_t* off, const int64_t* n,
                                     int32_t sample_rate, const nc_loudness_cfg* cfg, nc_loudness_row* out, void* hip_stream) {
    return guard([&] {
        if (!pcm || !out) fail(NC_EINVAL, "null pointer");
        const nc_loudness_cfg c = loudness_resolve_cfg(cfg, sample_rate);
        const int64_t* offs[1] = {off};
        loudness_check_clips(B, C, offs, 1, n);
        g_loud.locked(device_index, [&](LoudDev& q) {
            run_loudness(q, pcm, B, C, off, n, sample_rate, c, nullptr, nullptr, out, static_cast<hipStream_t>(hip_stream));
        });
    });
}

extern "C" nc_status nc_loudness_normalize_dev(int device_index, const float* pcm, int32_t B, int32_t C, const int64_t* off, const int64_t* n,
                                               int32_t sample_rate, const nc_loudness_cfg* cfg, float* out, const int64_t* out_off,
                                               nc_loudness_row* rows, void* hip_stream) {
    return guard([&] {
        if (!pcm || !out || !rows) fail(NC_EINVAL, "null pointer");
        const nc_loudness_cfg c = loudness_resolve_cfg(cfg, sample_rate);
        const int64_t* offs[2] = {off, out_off};
        loudness_check_clips(B, C, offs, 2, n);
        g_loud.locked(device_index, [&](LoudDev& q) {
            run_loudness(q, pcm, B, C, off, n, sample_rate, c, out, out_off, rows, static_cast<hipStream_t>(hip_stream));
        });
    });
}

extern "C" nc_status nc_audio_apply_gain_db_dev(int device_index, const float* pcm, int32_t B, int32_t C, const int64_t* off, const int64_t* n,
                                                const float* db, float* out, const int64_t* out_off, void* hip_stream) {
    return guard([&] {
        if (!pcm || !out) fail(NC_EINVAL, "null pointer");
        const int64_t* offs[2] = {off, out_off};
        loudness_check_clips(B, C, offs, 2, n);
        check_db(db, B);
        g_loud.locked(device_index, [&](LoudDev& q) { run_gain(q, pcm, B, C, off, n, db, out, out_off, static_cast<hipStream_t>(hip_stream)); });
    });
}

extern "C" nc_status nc_loudness(int device_index, const float* pcm, int32_t B, int32_t C, const int64_t* off, const int64_t* n, int32_t sample_rate,
                                 const nc_loudness_cfg* cfg, nc_loudness_row* out) {
    return guard([&] {
        if (!pcm || !out) fail(NC_EINVAL, "null pointer");
        const nc_loudness_cfg c = loudness_resolve_cfg(cfg, sample_rate);
        const int64_t* offs[1] = {off};
        loudness_check_clips(B, C, offs, 1, n);
        host_buffer_call(device_index, pcm, B, C, off, n, sample_rate, &c, nullptr, nullptr, nullptr, out);
    });
}

extern "C" nc_status nc_loudness_normalize(int device_index, const float* pcm, int32_t B, int32_t C, const int64_t* off, const int64_t* n,
                                           int32_t sample_rate, const nc_loudness_cfg* cfg, float* out, const int64_t* out_off,
                                           nc_loudness_row* rows) {
    return guard([&] {
        if (!pcm || !out || !rows) fail(NC_EINVAL, "null pointer");
        const nc_loudness_cfg c = loudness_resolve_cfg(cfg, sample_rate);
        const int64_t* offs[2] = {off, out_off};
        loudness_check_clips(B, C, offs, 2, n);
        host_buffer_call(device_index, pcm, B, C, off, n, sample_rate, &c, nullptr, out, out_off, rows);
    });
}

extern "C" nc_status nc_audio_apply_gain_db(int device_index, const float* pcm, int32_t B, int32_t C, const int64_t* off, const int64_t* n,
                                            const float* db, float* out, const int64_t* out_off) {
    return guard([&] {
        if (!pcm || !out) fail(NC_EINVAL, "null pointer");
        const int64_t* offs[2] = {off, out_off};
        loudness_check_clips(B, C, offs, 2, n);
        check_db(db, B);
        host_buffer_call(device_index, pcm, B, C, off, n, 0, nullptr, db, out, out_off, nullptr);
    });
}
