// Encodec on the engine: the SEANet encoder / decoder driver, its element kernels (pad, GroupNorm sums, RMS scale) and the overlap-add.
// The LSTM is nc_lstm.hip, the Euclidean RVQ nc_euclid_rvq.hip, the streaming convolutions nc_resa / nc_down2 / nc_down_s / nc_up2.hip.
//
// Reference call stacks restated as kernel launches:
//   Encodec.Encode  Models/Encodec.cs:259-285 -> EncodeFrame :457-489 -> SEANetEncoder.cs:37-148 -> ResidualVectorQuantizer.cs:133-157
//   Encodec.Decode  Models/Encodec.cs:213-235 -> DecodeFrame :436-455 -> SEANetDecoder.cs:40-153 -> DSP.LinearOverlapAdd
// An activation is written ONCE, raw, with its GroupNorm pending (Act): the consuming launch applies the normalisation, the ELU and the
// asymmetric reflect pad of SConv1d (SConv1d.cs:144-173, incl. the small-input path D9) while it stages its input, and the producing
// launch emits the GroupNorm block sums from its epilogue, the last workgroup of a sample to arrive finishing (mean, rstd).  The outer
// stages of the 48 kHz model run on the streaming kernels (a residual block's first pass in one launch; the stride-2 / 4 / 5 down- and
// stride-2 / 4 up-convolutions on both operands of the block in front of them).  A padded copy (pad_act_kernel) and the stand-alone
// GroupNorm passes (gn_block_kernel, gn_final_kernel) remain for the layers without such a form and behind the fallback switches.
// Dense contractions (convs, LSTM input projections) run on the matrix-core conv template; the recurrent part of an LSTM layer is one
// persistent launch over all its steps (per chunk of steps when the layers are pipelined).  Equal segments of a call run as one batch,
// the tail segment beside them on a side stream.
// Arithmetic is the canonical arithmetic of DESIGN.md (same sequences as oracle/c/nc_ref_encodec.c).
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "nc_gn.h"
#include "nc_math.h"
#include "nc_model.h"

namespace nc {

constexpr int GN_CHUNK = 256;    // RMS-scale chunks

// ---------------------------------------------------------------------------------------------- kernels
struct ActView {          // [B,C,L] view of a raw conv output with its pending GroupNorm (applied by the consumer)
    const float* p;
    int64_t rs, off;      // row stride (elements), offset of logical sample 0 in a row (conv-transpose trim)
    const float* stats;   // [B][2] = (mean, rstd); null: no normalisation
    const float* gamma;
    const float* beta;
};

__device__ __forceinline__ float act_value(const ActView& v, int64_t b, int c, int C, int64_t q) {
    float x = v.p[(b * C + c) * v.rs + v.off + q];
    if (v.stats) x = ((x - v.stats[2 * b]) * v.stats[2 * b + 1]) * v.gamma[c] + v.beta[c];
    return x;
}

// dst[b,c,j] = pad(elu?(GN(a) [+ GN(b2)]))[j],  j in [0,Lp): reflect over the zero-extended row of length Lz (SConv1d.cs:258-274).
// Grid = (row segments of 1024, channels, samples): no index division, the per-(b,c) operands are scalars, 4 elements per thread
// with all reads ahead of the stores.
__global__ __launch_bounds__(256) void pad_act_kernel(ActView a, ActView b2, int has_b, int elu, float* __restrict__ dst, int C, int64_t L, int64_t Lz,
                                                      int64_t left, int64_t Lp) {
    const int c = blockIdx.y;
    const int64_t b = blockIdx.z;
    const float* ra = a.p + (b * C + c) * a.rs + a.off;
    const float* rb = b2.p + (b * C + c) * b2.rs + b2.off;
    const bool na = a.stats != nullptr, nb = has_b && b2.stats != nullptr;
    const float mu_a = na ? a.stats[2 * b] : 0.0f, r_a = na ? a.stats[2 * b + 1] : 1.0f, g_a = na ? a.gamma[c] : 1.0f, be_a = na ? a.beta[c] : 0.0f;
    const float mu_b = nb ? b2.stats[2 * b] : 0.0f, r_b = nb ? b2.stats[2 * b + 1] : 1.0f, g_b = nb ? b2.gamma[c] : 1.0f, be_b = nb ? b2.beta[c] : 0.0f;
    float* out = dst + (b * C + c) * Lp;
    float va[4], vb[4];
    bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t j = (int64_t)blockIdx.x * 1024 + u * 256 + threadIdx.x;
        int64_t q = j - left;
        if (q < 0) q = -q;
        if (q >= Lz) q = 2 * (Lz - 1) - q;
        ok[u] = j < Lp && q >= 0 && q < L;
        const int64_t qa = ok[u] ? q : 0;
        va[u] = ra[qa];
        vb[u] = has_b ? rb[qa] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t j = (int64_t)blockIdx.x * 1024 + u * 256 + threadIdx.x;
        float v = va[u];
        if (na) v = ((v - mu_a) * r_a) * g_a + be_a;
        if (has_b) {
            float w = vb[u];
            if (nb) w = ((w - mu_b) * r_b) * g_b + be_b;
            v = v + w;
        }
        if (elu) v = nc_eluf(v);
        if (j < Lp) out[j] = ok[u] ? v : 0.0f;
    }
}

// Stand-alone GroupNorm block sums in the canonical order of nc_gn.h, for the outputs whose producing kernel cannot emit them from
// its epilogue (the streaming thin-output head, per-phase transposed launches): one wavefront per 32x32 block of the (rows = c*sub +
// t % sub, columns = t / sub) view of x [B][C][T]; lane (h, c) adds its 16 rows of column c, then the butterfly.
constexpr int GN_CBW = 4;   // column blocks per wavefront: their 64 row reads are all in flight before the first sum (memory-level parallelism)
__global__ __launch_bounds__(256) void gn_block_kernel(const float* __restrict__ x, double* __restrict__ part, int64_t B, int C, int64_t T, int sub,
                                                       int nrb, int ncb, int64_t rs /* row pitch (elements) */) {
    const int lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
    const int ncg = (ncb + GN_CBW - 1) / GN_CBW;                      // groups of column blocks per row block
    const int64_t total = B * nrb * ncg;
    const int64_t gi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gi >= total) return;
    const int64_t b = gi / ((int64_t)nrb * ncg), rem = gi - b * nrb * ncg;
    const int rb = (int)(rem / ncg), cg = (int)(rem - (int64_t)rb * ncg);
    const float* xb = x + b * C * rs;
    float v[GN_CBW][16];
    unsigned okm[GN_CBW];
#pragma unroll
    for (int u = 0; u < GN_CBW; ++u) {
        const int64_t q = (int64_t)(cg * GN_CBW + u) * 32 + c;
        okm[u] = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int R = rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            const int co = sub == 1 ? R : R / sub;
            const int64_t t = sub == 1 ? q : q * sub + (R - co * sub);
            const bool ok = co < C && t < T;
            v[u][r] = xb[(int64_t)min(co, C - 1) * rs + min(t, T - 1)];   // branch-free: clamped address, value masked in the sum
            if (ok) okm[u] |= 1u << r;
        }
    }
#pragma unroll
    for (int u = 0; u < GN_CBW; ++u) {
        const int cb = cg * GN_CBW + u;
        double s1, s2;
        nc_gn_slot_sums<false>(v[u], okm[u], s1, s2);
        nc_gn_butterfly(s1, s2);
        if (lane == 0 && cb < ncb) {
            const int64_t bi = (b * nrb + rb) * ncb + cb;
            part[2 * bi] = s1;
            part[2 * bi + 1] = s2;
        }
    }
}
// one wavefront per sample: the n block sums of the sample by 64 strided slots (slot i: idx = i, i+64, ... ascending) + butterfly
// -> (mean, rstd); count = C*T elements
__global__ __launch_bounds__(64) void gn_final_kernel(const double* __restrict__ part, float* __restrict__ stats, int64_t n, double count) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const double* p = part + 2 * (int64_t)b * n;
    double s1 = 0.0, s2 = 0.0;
    for (int64_t k0 = 0; k0 < n; k0 += 64 * 8) {   // 8 independent 16-byte reads in flight per lane
        double a[8], c[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int64_t k = k0 + lane + 64 * u;
            const double2 v = k < n ? *reinterpret_cast<const double2*>(p + 2 * k) : double2{0.0, 0.0};
            a[u] = v.x; c[u] = v.y;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) { s1 += a[u]; s2 += c[u]; }
    }
    nc_gn_butterfly(s1, s2);
    if (lane == 0) {
        const double mu = s1 / count;
        double var = s2 / count - mu * mu;
        if (var < 0.0) var = 0.0;
        stats[2 * b] = (float)mu;
        stats[2 * b + 1] = (float)(1.0 / sqrt(var + 1e-5));
    }
}

// RMS scale (Encodec.cs:469-480): chunk sums of fl32(mono^2), then scale = sqrtf((float)(S/L)) + 1e-8f
__global__ void rms_partial_kernel(const float* __restrict__ x, double* __restrict__ part, int B, int C, int64_t L, int nchunk) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= (int64_t)B * nchunk) return;
    const int64_t b = i / nchunk, ch = i - b * nchunk;
    const int64_t t0 = ch * GN_CHUNK, t1 = t0 + GN_CHUNK < L ? t0 + GN_CHUNK : L;
    double s = 0.0;
    for (int64_t t = t0; t < t1; ++t) {
        float a = x[(b * C) * L + t];
        for (int c = 1; c < C; ++c) a = a + x[(b * C + c) * L + t];
        const float m = a / (float)C;
        s += (double)(m * m);
    }
    part[i] = s;
}
__global__ void rms_final_kernel(const double* __restrict__ part, float* __restrict__ scale, int B, int64_t L, int nchunk) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    double s = 0.0;
    for (int k = 0; k < nchunk; ++k) s += part[(int64_t)b * nchunk + k];
    scale[b] = sqrtf((float)(s / (double)L)) + 1e-8f;
}
// The same scale in ONE launch (the default; NC_RMS_TWO_PASS=1 runs the two kernels above): a workgroup stages RMS_G chunks of a clip through
// LDS -- coalesced reads, fl32(mono^2) per sample computed in parallel -- and thread g adds chunk g's 256 values in ascending order in
// binary64 (the canonical chunk sum); the LAST workgroup of a clip to arrive (self-resetting counter, the hand-off of nc_gn.h: write-through
// partials, drain, barrier, one relaxed agent-scope fetch-add, agent-scope loads) adds the clip's chunk sums in ascending order and writes
// the scale.  Bit-identical to rms_partial_kernel + rms_final_kernel: 44 + 24 us -> one short launch on C3 (16 x 2 s).
constexpr int RMS_G = 16;
__global__ __launch_bounds__(256) void rms_scale_kernel(const float* __restrict__ x, double* __restrict__ part, unsigned* __restrict__ counter,
                                                        float* __restrict__ scale, int C, int64_t L, int nchunk, int nblk) {
    __shared__ float sq[RMS_G][GN_CHUNK + 1];
    __shared__ double fin[256];
    __shared__ int last;
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk, tid = threadIdx.x;
    const int64_t t_base = (int64_t)blk * RMS_G * GN_CHUNK;
    const float* xb = x + (int64_t)b * C * L;
    const float invC = (float)C;
    for (int g0 = 0; g0 < RMS_G; g0 += 4) {                       // four chunk rows per pass: the reads of a pass are in flight together
        float a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t t = t_base + (int64_t)(g0 + u) * GN_CHUNK + tid;
            a[u] = t < L ? xb[t] : 0.0f;
        }
        for (int c = 1; c < C; ++c) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t t = t_base + (int64_t)(g0 + u) * GN_CHUNK + tid;
                const float v = t < L ? xb[(int64_t)c * L + t] : 0.0f;
                a[u] = a[u] + v;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float m = a[u] / invC;
            sq[g0 + u][tid] = m * m;
        }
    }
    __syncthreads();
    const int ch = blk * RMS_G + tid;
    if (tid < RMS_G && ch < nchunk) {
        const int64_t t0 = (int64_t)ch * GN_CHUNK;
        const int n = (int)((t0 + GN_CHUNK < L ? t0 + GN_CHUNK : L) - t0);
        double acc = 0.0;
        for (int i = 0; i < n; ++i) acc += (double)sq[tid][i];
        __hip_atomic_store(part + (int64_t)b * nchunk + ch, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) last = __hip_atomic_fetch_add(counter + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1 == (unsigned)nblk;
    __syncthreads();
    if (!last) return;
    double tot = 0.0;                                               // (ascending chunk order, one accumulator: rms_final_kernel's sum)
    for (int k0 = 0; k0 < nchunk; k0 += 256) {
        if (k0 + tid < nchunk) fin[tid] = __hip_atomic_load(part + (int64_t)b * nchunk + k0 + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (tid == 0) {
            const int n = nchunk - k0 < 256 ? nchunk - k0 : 256;
            for (int i = 0; i < n; ++i) tot += fin[i];
        }
        __syncthreads();
    }
    if (tid == 0) {
        scale[b] = sqrtf((float)(tot / (double)L)) + 1e-8f;
        __hip_atomic_store(counter + b, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// y = x / scale[b]  (mode 0)   |   y = GN(x) * scale[b] (mode 1, scale nullable -> plain GN materialisation)
__global__ void scale_kernel(ActView a, const float* __restrict__ scale, int mode, float* __restrict__ y, int B, int C, int64_t L) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * C * L) return;
    const int64_t t = i % L, r = i / L;
    const int c = (int)(r % C);
    const int64_t b = r / C;
    float v = act_value(a, b, c, C, t);
    if (scale) v = mode == 0 ? v / scale[b] : v * scale[b];
    y[i] = v;
}

// DSP.LinearOverlapAdd (AudioTensorDSP.cs:161-261): out[r,i] = (sum_f frame_f[r, i - f*stride] * w[i - f*stride]) / sw[i]
// Frame pointers / lengths come from device arrays (any number of segments); only the frames that can cover sample t are visited,
// in ascending order -- the same additions the all-frames loop performs.
__global__ void overlap_add_kernel(const float* const* __restrict__ fp, const int64_t* __restrict__ flen, int nfr, int64_t L0,
                                   const float* __restrict__ w, const float* __restrict__ sw, int64_t rows, int64_t stride, int64_t total,
                                   float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * total) return;
    const int64_t r = i / total, t = i - r * total;
    const int64_t f_lo = t >= L0 ? (t - L0) / stride + 1 : 0;
    const int64_t f_hi = min((int64_t)nfr - 1, t / stride);
    float a = 0.0f;
    for (int64_t f = f_lo; f <= f_hi; ++f) {
        const int64_t q = t - f * stride, len = flen[f];
        if (q >= 0 && q < len) a = a + fp[f][r * len + q] * w[q];
    }
    out[i] = a / sw[t];
}

// ---------------------------------------------------------------------------------------------- model
EncodecModel::EncodecModel(const nc_encodec_config& c) : cfg(c) {
    if (c.n_ratios <= 0 || c.n_ratios > 8) fail(NC_EINVAL, "ratios must hold 1..8 entries");
    if (c.channels <= 0 || c.channels > 2) fail(NC_EINVAL, "Invalid number of channels: %d", c.channels);          // Encodec.cs:267-270
    if (c.dimension <= 0 || c.dimension > EUCLID_MAX_D || c.n_filters <= 0 || c.sample_rate <= 0 || c.codebook_size <= 0 || c.n_codebooks <= 0 ||
        c.n_codebooks > 64 || c.frame_rate <= 0 || c.lstm_layers < 0 || c.lstm_layers > 4 || c.compress <= 0)
        fail(NC_EINVAL, "Encodec config fields out of range");
    if (c.kernel_size != 7 || c.last_kernel_size != 7 || c.residual_kernel_size != 3)
        fail(NC_EUNSUPPORTED, "SEANet kernel sizes other than 7/7/3 are not instantiated");
    if (c.time_group_norm && c.causal) fail(NC_EINVAL, "GroupNorm doesn't support causal evaluation");               // NormConv1d.cs:143-147
    if ((c.segment_length > 0) != (c.segment_stride > 0)) fail(NC_EINVAL, "segment_length and segment_stride go together");
    hop = 1;
    for (int i = 0; i < c.n_ratios; ++i) {
        if (c.ratios[i] <= 0) fail(NC_EINVAL, "ratios must be positive");
        hop *= c.ratios[i];
    }
    set_bandwidth(c.bandwidth);
}

void EncodecModel::set_bandwidth(float bw) {
    // ResidualVectorQuantizer.Encode (:139-147): nQ = max(1, floor(bw*1000 / (log2(bins)*frameRate)))
    const double bw_per_q = std::log2((double)cfg.codebook_size) * cfg.frame_rate;
    int n = cfg.n_codebooks;
    if (bw > 0) n = (int)std::max(1.0, std::floor((double)bw * 1000.0 / bw_per_q));
    if (n > cfg.n_codebooks) fail(NC_EINVAL, "This model doesn't support the bandwidth %g kbps", (double)bw);          // Encodec.cs:411-416
    n_q = n;
    cfg.bandwidth = bw;
}

EncodecModel::Plan EncodecModel::plan_sconv(int64_t L, int k, int stride, int dil) const {
    Plan p;
    const int64_t eff = (int64_t)(k - 1) * dil + 1, pt = eff - stride;
    const float nf = (float)(L - eff + pt) / (float)stride + 1.0f;                      // SConv1d.cs:245-250 (float division)
    const int64_t ideal = ((int64_t)std::ceil(nf) - 1) * stride + (eff - pt);
    const int64_t extra = ideal - L;
    if (cfg.causal) { p.left = pt; p.right = extra; }
    else { const int64_t r = pt / 2; p.left = pt - r; p.right = r + extra; }
    const int64_t mx = std::max(p.left, p.right);
    p.Lz = L <= mx ? L + (mx - L + 1) : L;                                                 // SConv1d.cs:258-274 (D9)
    p.Lp = p.Lz + p.left + p.right;
    p.Lout = (p.Lp - eff) / stride + 1;
    return p;
}

int64_t EncodecModel::frames_for(int64_t L) const {
    L = plan_sconv(L, cfg.kernel_size, 1, 1).Lout;
    for (int i = cfg.n_ratios - 1; i >= 0; --i) {
        L = plan_sconv(L, cfg.residual_kernel_size, 1, 1).Lout;
        L = plan_sconv(L, 2 * cfg.ratios[i], cfg.ratios[i], 1).Lout;
    }
    return plan_sconv(L, cfg.last_kernel_size, 1, 1).Lout;
}
int64_t EncodecModel::decoded_for(int64_t Tz) const {
    int64_t L = plan_sconv(Tz, cfg.kernel_size, 1, 1).Lout;
    for (int i = 0; i < cfg.n_ratios; ++i) {
        L = L * cfg.ratios[i];
        L = plan_sconv(L, cfg.residual_kernel_size, 1, 1).Lout;
    }
    return plan_sconv(L, cfg.last_kernel_size, 1, 1).Lout;
}

std::vector<EncodecModel::Seg> EncodecModel::segments(int64_t T) const {
    std::vector<Seg> v;
    const int64_t seg = cfg.segment_length > 0 ? cfg.segment_length : T, stride = cfg.segment_stride > 0 ? cfg.segment_stride : T;
    for (int64_t off = 0; off < T; off += stride) {                                         // Encodec.cs:278-282
        Seg s;
        s.off = off;
        s.len = std::min(off + seg, T) - off;
        s.frames = frames_for(s.len);
        v.push_back(s);
    }
    return v;
}

void EncodecModel::load_sconv(const Blob& b, const std::string& key, SConv& L, int Cin, int Cout, int K, int stride, bool transposed) {
    const BlobTensor* w = b.find(key + ".conv.weight");
    const BlobTensor* bias = b.find(key + ".conv.bias");
    const int64_t d0 = transposed ? Cin : Cout, d1 = transposed ? Cout : Cin;
    std::vector<float> folded;
    const float* dense;
    if (w) {
        if (w->dims.size() != 3 || w->dims[0] != d0 || w->dims[1] != d1 || w->dims[2] != K) fail(NC_EINVAL, "%s.conv.weight has the wrong shape", key.c_str());
        dense = static_cast<const float*>(w->data);
    } else {
        const BlobTensor& v = b.get(key + ".conv.weight_v");
        const BlobTensor& g = b.get(key + ".conv.weight_g");
        if (v.dims.size() != 3 || v.dims[0] != d0 || v.dims[1] != d1 || v.dims[2] != K || g.numel() != d0)
            fail(NC_EINVAL, "%s.conv.weight_v/g have the wrong shape", key.c_str());
        folded.resize((size_t)v.numel());
        fold_weight_norm_snac(static_cast<const float*>(v.data), static_cast<const float*>(g.data), d0, d1 * K, folded.data());   // D3
        dense = folded.data();
    }
    if (bias && bias->numel() != Cout) fail(NC_EINVAL, "%s.conv.bias has the wrong length", key.c_str());
    L.K = K; L.stride = stride; L.Cin = Cin; L.Cout = Cout; L.transposed = transposed;
    L.conv.kclass = transposed ? NC_KC_CONV_UP : (stride > 1 ? NC_KC_CONV_DOWN : (K == 1 ? NC_KC_CONV_K1 : (Cin <= 2 ? NC_KC_STEM : (Cout <= 2 ? NC_KC_HEAD : NC_KC_CONV_MISC))));
    L.conv.build(dense, bias ? static_cast<const float*>(bias->data) : nullptr, Cin, Cout, K, stride, 0, 1, 0, transposed);
    if (cfg.time_group_norm) {
        const BlobTensor& gw = b.get(key + ".norm.weight");
        const BlobTensor& gb = b.get(key + ".norm.bias");
        if (gw.numel() != Cout || gb.numel() != Cout) fail(NC_EINVAL, "%s.norm has the wrong shape", key.c_str());
        upload_f32(L.gamma, static_cast<const float*>(gw.data), Cout);
        upload_f32(L.beta, static_cast<const float*>(gb.data), Cout);
    }
}

void EncodecModel::load_resblock(const Blob& b, const std::string& key, ResBlock& r, int dim) {
    const int h = dim / cfg.compress;
    load_sconv(b, key + ".block.1", r.c1, dim, h, cfg.residual_kernel_size, 1, false);
    load_sconv(b, key + ".block.3", r.c2, h, dim, 1, 1, false);
    load_sconv(b, key + ".shortcut", r.sc, dim, dim, 1, 1, false);
}

void EncodecModel::load(const Blob& b) {
    use_device();
    char nm[128];
    const int nf = cfg.n_filters;
    load_sconv(b, "encoder.layers.0", enc_in, cfg.channels, nf, cfg.kernel_size, 1, false);
    int n = 1, mult = 1;
    for (int i = 0; i < cfg.n_ratios; ++i) {
        const int r = cfg.ratios[cfg.n_ratios - 1 - i], d = mult * nf;
        snprintf(nm, sizeof nm, "encoder.layers.%d", n);
        load_resblock(b, nm, enc_res[i], d);
        snprintf(nm, sizeof nm, "encoder.layers.%d", n + 2);
        load_sconv(b, nm, enc_down[i], d, 2 * d, 2 * r, r, false);
        n += 3;
        mult *= 2;
    }
    snprintf(nm, sizeof nm, "encoder.layers.%d", n);
    load_lstm(b, nm, enc_lstm, mult * nf, cfg.lstm_layers);
    snprintf(nm, sizeof nm, "encoder.layers.%d", n + 2);
    load_sconv(b, nm, enc_out, mult * nf, cfg.dimension, cfg.last_kernel_size, 1, false);
    books.clear();
    book_tab = EuclidBooks();
    for (int i = 0; i < cfg.n_codebooks; ++i) {
        snprintf(nm, sizeof nm, "quantizer.layers.%d.codebook.embed", i);
        const BlobTensor& e = b.get(nm);
        if (e.dims.size() != 2 || e.dims[0] != cfg.codebook_size || e.dims[1] != cfg.dimension) fail(NC_EINVAL, "%s has the wrong shape", nm);
        books.emplace_back(new Codebook());
        books.back()->build(static_cast<const float*>(e.data), cfg.codebook_size, cfg.dimension);
        book_tab.add(*books.back());
    }
    book_tab.upload();
    load_sconv(b, "decoder.layers.0", dec_in, cfg.dimension, mult * nf, cfg.kernel_size, 1, false);
    load_lstm(b, "decoder.layers.1", dec_lstm, mult * nf, cfg.lstm_layers);
    n = 2;
    for (int i = 0; i < cfg.n_ratios; ++i) {
        const int r = cfg.ratios[i], d = mult * nf;
        snprintf(nm, sizeof nm, "decoder.layers.%d", n + 1);
        load_sconv(b, nm, dec_up[i], d, d / 2, 2 * r, r, true);
        snprintf(nm, sizeof nm, "decoder.layers.%d", n + 2);
        load_resblock(b, nm, dec_res[i], d / 2);
        n += 3;
        mult /= 2;
    }
    snprintf(nm, sizeof nm, "decoder.layers.%d", n + 1);
    load_sconv(b, nm, dec_out, nf, cfg.channels, cfg.last_kernel_size, 1, false);
    gn_counters.reserve((size_t)3 * 2 * GN_MAX_SAMPLES * sizeof(unsigned));
    NC_HIP(hipMemset(gn_counters.p, 0, (size_t)3 * 2 * GN_MAX_SAMPLES * sizeof(unsigned)));
    lstm.prepare();
    if (!ev_fork) {
        for (int i = 0; i < 2; ++i) {
            NC_HIP(hipStreamCreateWithFlags(&side_stream[i], hipStreamNonBlocking));
            NC_HIP(hipEventCreateWithFlags(&ev_join[i], hipEventDisableTiming));
        }
        NC_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    }
    NC_HIP(hipDeviceSynchronize());
    loaded = true;
}

EncodecModel::~EncodecModel() {
    for (int i = 0; i < 2; ++i) {
        if (side_stream[i]) (void)hipStreamDestroy(side_stream[i]);
        if (ev_join[i]) (void)hipEventDestroy(ev_join[i]);
    }
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    for (hipEvent_t e : ola.ev)
        if (e) (void)hipEventDestroy(e);
    if (ola.pin) (void)hipHostFree(ola.pin);
}

// Called where the host knows the stream is idle (nc_codec_synchronize, the host-pointer entry points, nc_codec_check_errors) and at the
// start of every device-pointer call: a persistent LSTM launch that timed out invalidated the call it belonged to.  The handle then
// switches to the step-wise kernels (fresh launches need no co-residency), so the caller's retry -- or, for the host-pointer entry
// points, the engine's own -- succeeds.
void EncodecModel::check_async_errors() {
    if (lstm.note_timeout())
        fail(NC_EDEVICE, "persistent LSTM kernel: a workgroup exchange timed out (its workgroups were not co-resident); the results of that call are "
                         "invalid -- this handle now runs the step-wise LSTM kernels, repeat the call");
}

// ---- launch helpers --------------------------------------------------------------------------------
float* EncodecModel::alloc(size_t n_floats) {
    const size_t idx = pool_i++ * (size_t)pool_lanes + (size_t)pool_lane;
    while (pool.size() <= idx) pool.emplace_back(new DevBuf());
    pool[idx]->reserve(n_floats * sizeof(float));
    return pool[idx]->as<float>();
}

static ActView view_of(const EncodecModel::Act& a) {
    ActView v;
    v.p = a.p; v.rs = a.rs; v.off = a.off; v.stats = a.stats; v.gamma = a.gamma; v.beta = a.beta;
    return v;
}

float* EncodecModel::pad_act(const Act& a, const Act* b2, bool elu, int N, const Plan& pl) {
    float* dst = alloc((size_t)N * a.C * pl.Lp);
    ActView vb = b2 ? view_of(*b2) : view_of(a);
    {
        ProfScope ps(&prof, stream, NC_KC_ELEM, 0.0, 4.0 * N * a.C * ((double)a.L * (b2 ? 2 : 1) + (double)pl.Lp));
        hipLaunchKernelGGL(pad_act_kernel, dim3((unsigned)((pl.Lp + 1023) / 1024), (unsigned)a.C, (unsigned)N), dim3(256), 0, stream, view_of(a), vb,
                           b2 ? 1 : 0, elu ? 1 : 0, dst, a.C, a.L, pl.Lz, pl.left, pl.Lp);
    }
    NC_HIP(hipGetLastError());
    return dst;
}

// GroupNorm(1,C) statistics of a raw conv output [N,C,L] (NormConv1d.cs:155).  gn_begin sizes the block-sum buffer and, when the
// producing launch can emit the sums from its epilogue, hands the buffer to it (ConvIO::gn_part); gn_end runs the stand-alone block
// pass otherwise and then the per-sample final: (mean, rstd) pairs the consumer applies while staging its input.
EncodecModel::GnJob EncodecModel::gn_begin(const ConvLayer& conv, ConvIO& io, int N, int C, int64_t L, int sub) {
    GnJob j;
    if (!cfg.time_group_norm) return j;
    j.on = true; j.sub = sub;
    j.nrb = (int)(((int64_t)C * sub + 31) / 32);
    j.ncb = (int)(((L + sub - 1) / sub + 31) / 32);
    j.part = reinterpret_cast<double*>(alloc((size_t)N * j.nrb * j.ncb * 4));
    j.stats = alloc((size_t)N * 2);
    if (conv_gn_fusable(conv, io, N)) {
        io.gn_part = j.part; io.gn_nrb = j.nrb; io.gn_ncb = j.ncb;
        j.fused = true;
        // finish inside the launch: the last workgroup of a sample to arrive writes (mean, rstd).  One self-resetting counter per
        // sample; the segment groups of a call run concurrently, so each has its own set.
        if (gn_finishes_in_launch(N)) {
            io.gn_count = group_counters();
            io.gn_stats = j.stats;
            io.gn_n = gn_count_arg((double)C * (double)L);
            j.finished = true;
        }
    }
    return j;
}
const float* EncodecModel::gn_end(const GnJob& j, const float* raw, int N, int C, int64_t L, int64_t rs) {
    if (rs <= 0) rs = L;
    if (!j.on) return nullptr;
    if (FILE* lf = launch_log()) {   // where the statistics of this conv launch come from (tests/test_encodec_layers_gpu.py)
        std::fprintf(lf, "enc_gn %s\n", j.finished ? "epilogue_finished" : j.fused ? "epilogue_sums+final" : "block_pass+final");
        std::fflush(lf);
    }
    if (j.finished) return j.stats;
    const int64_t n = (int64_t)j.nrb * j.ncb;
    ProfScope ps(&prof, stream, NC_KC_NORM, 3.0 * N * C * (double)L, j.fused ? 16.0 * N * (double)n : 4.0 * N * C * (double)L);
    if (!j.fused)
        hipLaunchKernelGGL(gn_block_kernel, dim3((unsigned)(((int64_t)N * j.nrb * ((j.ncb + GN_CBW - 1) / GN_CBW) + 3) / 4)), dim3(256), 0, stream, raw, j.part,
                           (int64_t)N, C, L, j.sub, j.nrb, j.ncb, rs);
    hipLaunchKernelGGL(gn_final_kernel, dim3((unsigned)N), dim3(64), 0, stream, j.part, j.stats, n, (double)C * (double)L);
    NC_HIP(hipGetLastError());
    return j.stats;
}

static void fused_input(ConvIO& io, const EncodecModel::Act& a, bool elu, const EncodecModel::Plan* pl) {
    io.x = a.p + a.off; io.x_bstride = (int64_t)a.C * a.rs; io.x_cstride = a.rs;
    io.in_stats = a.stats; io.in_gamma = a.stats ? a.gamma : nullptr; io.in_beta = a.stats ? a.beta : nullptr;
    io.in_elu = elu;
    if (pl && (pl->left != 0 || pl->Lp != a.L)) {
        io.in_left = pl->left; io.in_Lz = pl->Lz; io.in_L = a.L;
        io.x_len = (int32_t)pl->Lp; io.Tin = pl->Lp;
    } else {
        io.x_len = (int32_t)a.L; io.Tin = a.L;
    }
}

// second operand of a two-input layer (the branch of a residual block beside its shortcut): same geometry, own pending GroupNorm
static void second_input(ConvIO& io, const EncodecModel::Act& b2) {
    io.x2 = b2.p + b2.off;
    io.in_stats2 = b2.stats; io.in_gamma2 = b2.stats ? b2.gamma : nullptr; io.in_beta2 = b2.stats ? b2.beta : nullptr;
}

// The streaming two-input kernels (Down2Args / Up2Args: same field names).  Operands: the two pending views with their GroupNorm triples.
template <class Args>
static void stream_operands(Args& d, const EncodecModel::Act& a, const EncodecModel::Act& b) {
    d.xa = a.p + a.off; d.xb = b.p + b.off; d.x_bstride = (int64_t)a.C * a.rs; d.x_cstride = a.rs;
    d.Cin = a.C;
    d.stats_a = a.stats; d.gamma_a = a.stats ? a.gamma : nullptr; d.beta_a = a.stats ? a.beta : nullptr;
    d.stats_b = b.stats; d.gamma_b = b.stats ? b.gamma : nullptr; d.beta_b = b.stats ? b.beta : nullptr;
}
// rows 8-byte aligned at even columns for both operands
template <class Args>
static bool stream_aligned(const Args& d) {
    auto al8 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 7) == 0; };
    return al8(d.xa) && al8(d.xb) && !(d.x_cstride & 1) && !(d.x_bstride & 1);
}
// GroupNorm block sums of the output (nrb x ncb blocks of 32 x 32 per clip) with the in-launch finish over `count` elements; alloc: the
// model's pool (partials first, then the [N][2] statistics, which it returns)
template <class Args, class Alloc>
static float* stream_gn_out(Args& d, int N, int nrb, int ncb, unsigned* counters, double count, Alloc&& alloc) {
    d.gn_nrb = nrb; d.gn_ncb = ncb;
    d.gn_part = reinterpret_cast<double*>(alloc((size_t)N * d.gn_nrb * d.gn_ncb * 4));
    float* st = alloc((size_t)N * 2);
    d.gn_stats = st;
    d.gn_count = counters;
    d.gn_n = gn_count_arg(count);
    return st;
}
// a raw tensor as a pending view: rows of `len` samples at pitch rs, starting `off` samples in; st: the [N][2] statistics of its pending
// GroupNorm, whose affine is layer L's (null: none pending)
static EncodecModel::Act make_act(const float* y, int C, int64_t len, int64_t rs, int64_t off, const float* st = nullptr, const EncodecModel::SConv* L = nullptr) {
    EncodecModel::Act o;
    o.p = y; o.C = C; o.L = len; o.rs = rs; o.off = off;
    o.stats = st; o.gamma = st && L ? L->gamma.as<float>() : nullptr; o.beta = st && L ? L->beta.as<float>() : nullptr;
    return o;
}
static EncodecModel::Act dense_act(const float* y, int C, int64_t len) { return make_act(y, C, len, len, 0); }

// NC_LAUNCH_LOG: one "enc_form <kernel> ..." line per launch of a streaming kernel (the form the driver took, for tests/test_encodec_layers_gpu.py)
static void log_enc_form(const char* kernel, int p, bool aligned) {
    if (FILE* lf = launch_log()) {
        std::fprintf(lf, "enc_form %s<%d> %s\n", kernel, p, aligned ? "aligned" : "unaligned");
        std::fflush(lf);
    }
}

// two operands one launch can read side by side: same shape and pitch, both or neither with a pending GroupNorm
static bool same_geometry(const EncodecModel::Act& a, const EncodecModel::Act& b) {
    return b.C == a.C && b.L == a.L && b.rs == a.rs && (a.stats != nullptr) == (b.stats != nullptr);
}

bool EncodecModel::gn_finishes_in_launch(int N) const {
    static const bool no_finish = env_flag("NC_NO_GN_FINISH");
    return N <= GN_MAX_SAMPLES && !no_finish;
}

// the stride-2 / stride-4 / stride-5 down-convolutions behind the residual blocks: streaming two-input kernels (nc_down2.hip, nc_down_s.hip)
bool EncodecModel::try_stream_down(SConv& L, const Act& a, const Act* b2, bool elu, int N, const Plan& pl, Act& out) {
    static const bool no_down2 = env_flag("NC_NO_DOWN2");
    static const bool no_down4 = env_flag("NC_NO_DOWN4");
    static const bool no_down5 = env_flag("NC_NO_DOWN5");
    const int64_t T = a.L;
    const bool common = b2 && elu && !cfg.causal && !L.transposed && !(L.Cin & 1) && L.Cin <= 128 && same_geometry(a, *b2) &&
                        pl.Lz == T && (int64_t)(a.C + 1) * a.rs + T < ((int64_t)1 << 32) && (!cfg.time_group_norm || gn_finishes_in_launch(N));
    auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    const bool s2 = common && !no_down2 && L.K == 4 && L.stride == 2 && L.conv.cfg.TM == 2 && L.conv.cfg.CB == 8 && L.Cout == 64 && T >= 4 && !(T & 1) &&
                    pl.left == 1 && pl.right == 1 && pl.Lout == T / 2;
    const bool s4 = common && !no_down4 && L.K == 8 && L.stride == 4 && L.conv.cfg.TM == 4 && L.conv.cfg.CB == 4 && L.Cout == 128 && L.Cin % 8 == 0 && T >= 8 &&
                    !(T & 3) && pl.left == 2 && pl.right == 2 && pl.Lout == T / 4 && !(a.rs & 3) && al16(a.p + a.off) && al16(b2->p + b2->off);
    const bool s5 = common && !no_down5 && L.K == 10 && L.stride == 5 && L.conv.cfg.TM == 4 && L.conv.cfg.CB == 3 && L.Cout == 256 && L.Cin % 4 == 0 && T >= 10 &&
                    T % 5 == 0 && pl.left == 3 && pl.right == 2 && pl.Lout == T / 5;
    if (!(s2 || s4 || s5)) return false;
    Down2Args d{};
    stream_operands(d, a, *b2);
    d.T = (int)T; d.Tout = (int)pl.Lout;
    d.w = L.conv.w.as<float>(); d.bias = L.conv.has_bias ? L.conv.bias.as<float>() : nullptr;
    float* y = alloc((size_t)N * L.Cout * pl.Lout);
    d.y = y; d.y_bstride = (int64_t)L.Cout * pl.Lout; d.y_cstride = pl.Lout; d.Cout = L.Cout;
    d.B = N; d.n_t_tiles = (int)((pl.Lout + 127) / 128); d.n_cb = (L.Cin + 7) / 8;   // (both kernels walk 8 input channels per barrier; the stride-4 one = two blocks of its CB = 4 image)
    d.n_co_tiles = 1; d.w_co_stride = 0;
    if (s5) {   // four channels per barrier; two row tiles of 128 whose images lie n_cb * KB * BM floats apart
        d.n_cb = L.Cin / 4; d.n_co_tiles = L.Cout / 128;
        d.w_co_stride = (int64_t)((L.Cin + 2) / 3) * 30 * 128;
    }
    float* st = nullptr;
    if (cfg.time_group_norm)
        st = stream_gn_out(d, N, L.Cout / 32, (int)((pl.Lout + 31) / 32), group_counters(), (double)L.Cout * (double)pl.Lout, [&](size_t n) { return alloc(n); });
    const bool aligned = stream_aligned(d);
    {
        ProfScope ps(&prof, stream, L.conv.kclass, L.conv.flops(N, pl.Lp), 4.0 * N * (2.0 * a.C * (double)T + (double)L.Cout * pl.Lout));
        if (!(s5 ? launch_down5(d, 4, stream) : s4 ? launch_down4(d, 4, stream) : launch_down2(d, 2, aligned, stream)))
            fail(NC_ESTATE, "internal: no streaming down-convolution instance");
    }
    log_enc_form("down", L.stride, s2 ? aligned : true);
    out = make_act(y, L.Cout, pl.Lout, pl.Lout, 0, st, &L);
    return true;
}

// SConv1d.forward on an activated view: returns the raw conv output with its pending GroupNorm.
// Single-input layers run with the producer's pending GroupNorm, the ELU and the asymmetric reflect pad folded into the conv's
// tile load (ConvArgs::in_mode): no padded copy of the activation is ever written.  Two-input layers (shortcut + branch of a
// residual block) take a streaming kernel or the two-input instances of the template where there is one; otherwise they are summed,
// activated and padded by pad_act_kernel first.
EncodecModel::Act EncodecModel::sconv(SConv& L, const Act& a, const Act* b2, bool elu, int N) {
    const Plan pl = plan_sconv(a.L, L.K, L.stride, 1);
    static const bool no_fuse = env_flag("NC_ENCODEC_NO_FUSE");
    Act o;
    if (!no_fuse && try_stream_down(L, a, b2, elu, N, pl, o)) return o;
    float* y = nullptr;
    ConvIO io{};
    const bool two_in = b2 && !no_fuse && conv_in2_available(L.conv) && same_geometry(a, *b2);
    if ((!b2 || two_in) && !no_fuse && pl.Lp < ((int64_t)1 << 30)) {
        fused_input(io, a, elu, &pl);
        if (two_in) second_input(io, *b2);
        y = alloc((size_t)N * L.Cout * pl.Lout);
    } else {
        const bool passthrough = !b2 && !elu && !a.stats && pl.left == 0 && pl.Lp == a.L && a.off == 0 && a.rs == a.L;
        const float* xin = passthrough ? a.p : pad_act(a, b2, elu, N, pl);
        y = alloc((size_t)N * L.Cout * pl.Lout);
        io.x = xin; io.x_bstride = (int64_t)L.Cin * pl.Lp; io.x_cstride = pl.Lp; io.x_len = (int32_t)pl.Lp; io.Tin = pl.Lp;
    }
    io.y = y; io.y_bstride = (int64_t)L.Cout * pl.Lout; io.y_cstride = pl.Lout;
    const GnJob gj = gn_begin(L.conv, io, N, L.Cout, pl.Lout, 1);
    launch_conv(L.conv, io, N, stream, &prof);
    return make_act(y, L.Cout, pl.Lout, pl.Lout, 0, gn_end(gj, y, N, L.Cout, pl.Lout), &L);
}

// the stride-2 / stride-4 up-convolutions in front of the last two residual blocks: streaming two-input kernel (nc_up2.hip)
bool EncodecModel::try_stream_up(SConv& L, const Act& a, const Act* b2, bool elu, int N, Act& out) {
    static const bool no_up2 = env_flag("NC_NO_UP2");
    static const bool no_up4 = env_flag("NC_NO_UP4");
    const int64_t T = a.L, Lfull = (a.L - 1) * L.stride + L.K;
    const int S = L.stride;
    const bool common = b2 && !cfg.causal && L.transposed && L.K == 2 * S && L.conv.sub_stride == S && L.conv.n_phase == 1 && L.conv.cfg.CB == 16 &&
                        !(L.Cin & 1) && L.Cin <= 128 && same_geometry(a, *b2) &&
                        T >= 4 && !(T & 1) && (int64_t)(a.C + 1) * a.rs + T < ((int64_t)1 << 32) && (int64_t)L.Cout * Lfull < ((int64_t)1 << 31) &&
                        (!cfg.time_group_norm || gn_finishes_in_launch(N));
    const bool u2 = common && !no_up2 && S == 2 && L.conv.cfg.TM == 2 && L.Cout == 32;
    const bool u4 = common && !no_up4 && S == 4 && L.conv.cfg.TM == 4 && L.Cout == 64;
    if (!(u2 || u4)) return false;
    Up2Args d{};
    stream_operands(d, a, *b2);
    d.L = (int)T; d.elu = elu ? 1 : 0;
    d.w = L.conv.w.as<float>(); d.bias = L.conv.has_bias ? L.conv.bias.as<float>() : nullptr;
    float* y = alloc((size_t)N * L.Cout * Lfull);
    d.y = y; d.y_bstride = (int64_t)L.Cout * Lfull; d.y_cstride = Lfull; d.Cout = L.Cout;
    d.B = N; d.n_t_tiles = (int)((T + 1 + 255) / 256); d.n_cb = (L.Cin + 15) / 16; d.n_co_tiles = S * L.Cout / (32 * L.conv.cfg.TM);
    float* st = nullptr;
    if (cfg.time_group_norm)
        st = stream_gn_out(d, N, S * L.Cout / 32, (int)(((Lfull + S - 1) / S + 31) / 32), group_counters(), (double)L.Cout * (double)Lfull,
                           [&](size_t n) { return alloc(n); });
    const bool aligned = stream_aligned(d);
    {
        ProfScope ps(&prof, stream, L.conv.kclass, L.conv.flops(N, T), 4.0 * N * (2.0 * a.C * (double)T + (double)L.Cout * Lfull));
        if (!launch_up2(d, L.conv.cfg.TM, S, aligned, stream)) fail(NC_ESTATE, "internal: no streaming up-convolution instance");
    }
    log_enc_form("up", S, aligned);
    const int64_t pt = L.K - L.stride, right = pt / 2, left = pt - right;           // non-causal trim (SConvTranspose1d.cs:159-171)
    out = make_act(y, L.Cout, Lfull - left - right, Lfull, left, st, &L);
    return true;
}

// SConvTranspose1d.forward (SConvTranspose1d.cs:116-139): conv-transpose, GroupNorm over the UNTRIMMED output, then the trim
EncodecModel::Act EncodecModel::sconvT(SConv& L, const Act& a, const Act* b2, bool elu, int N) {
    static const bool no_fuse = env_flag("NC_ENCODEC_NO_FUSE");
    const int64_t Lfull = (a.L - 1) * L.stride + L.K;
    Act o;
    if (!no_fuse && try_stream_up(L, a, b2, elu, N, o)) return o;
    ConvIO io{};
    const bool two_in = b2 && !no_fuse && conv_in2_available(L.conv) && same_geometry(a, *b2);
    if ((!b2 || two_in) && !no_fuse) {
        fused_input(io, a, elu, nullptr);
        if (two_in) second_input(io, *b2);
    } else {
        Plan pl; pl.left = 0; pl.right = 0; pl.Lz = a.L; pl.Lp = a.L; pl.Lout = a.L;
        const float* xin = pad_act(a, b2, elu, N, pl);
        io.x = xin; io.x_bstride = (int64_t)L.Cin * a.L; io.x_cstride = a.L; io.x_len = (int32_t)a.L; io.Tin = a.L;
    }
    const int64_t pt = L.K - L.stride;
    int64_t right, left;
    if (cfg.causal) { right = pt; left = 0; }                                               // trimRightRatio = 1
    else { right = pt / 2; left = pt - right; }
    // The consumers read the TRIMMED view (rows start `left` samples in).  Where that start is not 8-byte aligned -- the stride-5 layer: left = 3,
    // odd row length 6005 -- the residual block behind it lost its aligned kernels (the C = 128 shortcut ran on the windowed template: 181 us
    // against 71 us for the same layer in the encoder).  Rows are therefore laid out at a pitch of whole 16 bytes and the buffer starts
    // `shift` samples in, so that every row of the trimmed view begins on a 16-byte boundary (NC_NO_UP_PITCH=1: dense rows, no shift).
    static const bool no_pitch = env_flag("NC_NO_UP_PITCH");
    const int64_t P = no_pitch ? Lfull : ((Lfull + 3) & ~(int64_t)3);
    const int64_t shift = no_pitch ? 0 : (4 - left % 4) % 4;
    float* y = alloc((size_t)N * L.Cout * P + 4) + shift;
    io.y = y; io.y_bstride = (int64_t)L.Cout * P; io.y_cstride = P;
    // (the block view of the statistics follows the layer geometry, not the kernel form: the same sums under NC_NO_SUBPIXEL)
    const GnJob gj = gn_begin(L.conv, io, N, L.Cout, Lfull, conv_gn_sub(L.K, L.stride, L.Cout, true));
    launch_conv(L.conv, io, N, stream, &prof);
    return make_act(y, L.Cout, Lfull - left - right, P, left, gn_end(gj, y, N, L.Cout, Lfull, P), &L);
}

// The first pass of a residual block as ONE launch (nc_resa.hip): s = shortcut(x) and h = conv3(elu(x)) from a single read of x -- the
// thin outer stages of the 48 kHz model (C = 32 / 64: HBM-bound; the block input was read twice, the k = 3 launch alone ran at 2.1 TB/s).
// Same arithmetic as the two launches (NC_NO_RES_A=1 runs those).
bool EncodecModel::resblock_first_pass(ResBlock& r, const Act& x, int N, Act& s, Act& h) {
    static const bool off = env_flag("NC_NO_RES_A") || env_flag("NC_ENCODEC_NO_FUSE");
    const int C = x.C;
    const int64_t T = x.L;
    if (off || cfg.causal || (C != 32 && C != 64) || r.sc.K != 1 || r.c1.K != 3 || r.sc.Cin != C || r.sc.Cout != C || r.c1.Cin != C || r.c1.Cout != C / 2) return false;
    if (r.sc.conv.cfg.TM != C / 32 || r.sc.conv.cfg.CB != 16 || r.c1.conv.cfg.TM != 1 || r.c1.conv.cfg.CB != 16) return false;   // one row tile each
    if (T < 4 || (T & 1) || T >= ((int64_t)1 << 30) || (int64_t)(C + 1) * x.rs + T >= ((int64_t)1 << 32)) return false;
    const Plan pl = plan_sconv(T, 3, 1, 1);
    if (pl.left != 1 || pl.Lz != T || pl.Lp != T + 2 || pl.Lout != T) return false;   // (the non-causal reflect pad 1 + 1 the kernel folds into its lanes)
    const bool gn = cfg.time_group_norm;
    if (gn && !gn_finishes_in_launch(N)) return false;
    float* ys = alloc((size_t)N * C * T);
    float* yb = alloc((size_t)N * (C / 2) * T);
    ResAArgs a{};
    a.x = x.p + x.off; a.x_bstride = (int64_t)x.C * x.rs; a.x_cstride = x.rs; a.Cin = C; a.T = (int)T;
    a.in_stats = x.stats; a.in_gamma = x.stats ? x.gamma : nullptr; a.in_beta = x.stats ? x.beta : nullptr;
    a.w_s = r.sc.conv.w.as<float>(); a.bias_s = r.sc.conv.has_bias ? r.sc.conv.bias.as<float>() : nullptr;
    a.ys = ys; a.ys_bstride = (int64_t)C * T; a.ys_cstride = T; a.Cs = C;
    a.w_b = r.c1.conv.w.as<float>(); a.bias_b = r.c1.conv.has_bias ? r.c1.conv.bias.as<float>() : nullptr;
    a.yb = yb; a.yb_bstride = (int64_t)(C / 2) * T; a.yb_cstride = T; a.Cb = C / 2;
    a.B = N; a.n_t_tiles = (int)((T + 255) / 256); a.n_cb = C / 16;
    float* st_s = nullptr; float* st_b = nullptr;
    if (gn) {
        a.gn_nrb_s = C / 32; a.gn_nrb_b = 1; a.gn_ncb = (int)((T + 31) / 32);
        a.gn_part_s = reinterpret_cast<double*>(alloc((size_t)N * a.gn_nrb_s * a.gn_ncb * 4));
        a.gn_part_b = reinterpret_cast<double*>(alloc((size_t)N * a.gn_nrb_b * a.gn_ncb * 4));
        st_s = alloc((size_t)N * 2); st_b = alloc((size_t)N * 2);
        a.gn_stats_s = st_s; a.gn_stats_b = st_b;
        a.gn_count_s = group_counters();
        a.gn_count_b = a.gn_count_s + GN_MAX_SAMPLES;
        a.gn_n_s = gn_count_arg((double)C * (double)T); a.gn_n_b = gn_count_arg((double)(C / 2) * (double)T);
    }
    auto al8 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 7) == 0; };
    const bool aligned = al8(a.x) && !(a.x_cstride & 1) && !(a.x_bstride & 1);
    {
        // (one class for the launch: the pointwise one -- 2/5 of its flops, all of its input bytes)
        ProfScope ps(&prof, stream, NC_KC_CONV_K1, 2.0 * C * (C + 1.5 * C) * (double)T * N, 4.0 * N * (double)T * (C + C + C / 2));
        if (!launch_res_a(a, C / 32, aligned, stream)) fail(NC_ESTATE, "internal: no first-pass kernel for C = %d", C);
    }
    log_enc_form("res_a", C / 32, aligned);
    s = make_act(ys, C, T, T, 0, st_s, &r.sc);
    h = make_act(yb, C / 2, T, T, 0, st_b, &r.c1);
    return true;
}

// SEANetResnetBlock.forward (:72-85): shortcut(x) + conv1(elu(conv3(elu(x)))) -> the two pending views (s, y)
void EncodecModel::resblock(ResBlock& r, const Act& x, int N, Act& s, Act& y) {
    Act h;
    if (!resblock_first_pass(r, x, N, s, h)) {
        s = sconv(r.sc, x, nullptr, false, N);
        h = sconv(r.c1, x, nullptr, true, N);
    }
    tap(s); tap(h);
    y = sconv(r.c2, h, nullptr, true, N);
    // A row shorter than the k=3 pad takes SConv1d's small-input path (zero-extend, never trimmed: D9), so the block branch comes
    // out LONGER than the 1x1 shortcut and the reference's add() would broadcast.  Such degenerate segments are rejected.
    if (y.L != s.L) fail(NC_EINVAL, "segment too short: a residual block sees %lld samples", (long long)x.L);
    tap(y);
}

// GroupNorm-apply of a view into a dense tensor (optionally x scale[b] / divided by scale[b])
float* EncodecModel::materialize(const Act& a, int N, const float* scale, int mode) {
    float* y = alloc((size_t)N * a.C * a.L);
    const int64_t n = (int64_t)N * a.C * a.L;
    hipLaunchKernelGGL(scale_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, view_of(a), scale, mode, y, N, a.C, a.L);
    NC_HIP(hipGetLastError());
    return y;
}

// SEANetEncoder.forward (SEANetEncoder.cs:37-148) on N rows
EncodecModel::Act EncodecModel::encoder_front(Act cur, int N) {
    cur = sconv(enc_in, cur, nullptr, false, N);
    tap(cur);
    for (int i = 0; i < cfg.n_ratios; ++i) {
        Act s, y;
        resblock(enc_res[i], cur, N, s, y);
        cur = sconv(enc_down[i], s, &y, true, N);
        tap(cur);
    }
    return cur;
}

EncodecModel::Act EncodecModel::encoder_stack(Act cur, int N) {
    cur = encoder_front(cur, N);
    const float* xl = materialize(cur, N, nullptr, 0);
    // (the ELU in front of the last convolution is applied by the LSTM's output store: once per element instead of once per row tile
    //  of the consumer's staging, and the consumer runs as a plain convolution)
    const bool lstm_elu = lstm_applies_elu(enc_lstm);
    const Act a = dense_act(lstm.run(enc_lstm, xl, N, cur.L, lstm_elu), cur.C, cur.L);
    tap(a, true, lstm_elu);
    Act e = sconv(enc_out, a, nullptr, !lstm_elu, N);
    tap(e);
    return e;
}

// EncodeFrame on N = clips of one segment length: x [N,channels,L] dense -> codes [N,n_q,T'] (+ scale [N], emb)
void EncodecModel::encode_batch(const float* x, int N, int64_t L, int64_t Tz, int64_t* codes, float* scale_out, float* emb_out) {
    Act cur = dense_act(x, cfg.channels, L);
    if (cfg.normalize) {
        const int nchunk = (int)((L + GN_CHUNK - 1) / GN_CHUNK);
        double* part = reinterpret_cast<double*>(alloc((size_t)N * nchunk * 2));
        float* sc = scale_out ? scale_out : alloc((size_t)N);
        static const bool two_pass = env_flag("NC_RMS_TWO_PASS");
        if (!two_pass && N <= GN_MAX_SAMPLES) {
            const int nblk = (nchunk + RMS_G - 1) / RMS_G;
            ProfScope ps(&prof, stream, NC_KC_ELEM, 3.0 * N * cfg.channels * (double)L, 4.0 * N * cfg.channels * (double)L);
            hipLaunchKernelGGL(rms_scale_kernel, dim3((unsigned)((int64_t)N * nblk)), dim3(256), 0, stream, x, part, group_counters(), sc, cfg.channels, L, nchunk, nblk);
        } else {
            hipLaunchKernelGGL(rms_partial_kernel, dim3((unsigned)(((int64_t)N * nchunk + 63) / 64)), dim3(64), 0, stream, x, part, N, cfg.channels, L, nchunk);
            hipLaunchKernelGGL(rms_final_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, stream, part, sc, N, L, nchunk);
        }
        cur.p = materialize(cur, N, sc, 0);
    }
    Act e = encoder_stack(cur, N);
    if (e.L != Tz) fail(NC_ESTATE, "internal: encoder produced %lld frames, expected %lld", (long long)e.L, (long long)Tz);
    float* residual = materialize(e, N, nullptr, 0);
    const int D = cfg.dimension;
    if (emb_out) NC_HIP(hipMemcpyAsync(emb_out, residual, (size_t)N * D * Tz * 4, hipMemcpyDeviceToDevice, stream));
    const int64_t total = (int64_t)N * Tz;
    if (prof.on) prof.begin(stream, NC_KC_RVQ, 2.0 * D * cfg.codebook_size * (double)total * n_q, 0.0);   // the distance GEMM
    launch_euclid_rvq(book_tab, n_q, -1, residual, N, Tz, codes, stream);
    if (prof.on) prof.end(stream);
}

// SEANetDecoder.forward (SEANetDecoder.cs:40-153) on N rows
EncodecModel::Act EncodecModel::decoder_stack(const float* emb, int N, int64_t Tz) {
    Act cur = sconv(dec_in, dense_act(emb, cfg.dimension, Tz), nullptr, false, N);
    tap(cur);
    const float* xl = materialize(cur, N, nullptr, 0);
    const bool lstm_elu = lstm_applies_elu(dec_lstm);
    Act s = dense_act(lstm.run(dec_lstm, xl, N, cur.L, lstm_elu), cur.C, cur.L);
    tap(s, true, lstm_elu);
    return decoder_tail(s, lstm_elu, N);
}

EncodecModel::Act EncodecModel::decoder_tail(Act s, bool lstm_elu, int N) {
    Act y;
    bool dual = false;
    for (int i = 0; i < cfg.n_ratios; ++i) {
        Act u = sconvT(dec_up[i], s, dual ? &y : nullptr, !(i == 0 && lstm_elu), N);
        tap(u);
        resblock(dec_res[i], u, N, s, y);
        dual = true;
    }
    Act o = sconv(dec_out, s, dual ? &y : nullptr, true, N);
    tap(o);
    return o;
}

// The test hook's tap (nc_model.h).  Shapes first, by the pad plans alone.
void EncodecModel::trace_shape(bool decoder, int64_t L, int tap_i, int* C_out, int64_t* L_out) const {
    if (L <= 0 || tap_i < 0 || tap_i >= trace_taps()) fail(NC_EINVAL, "tap %d of %d, rows of %lld", tap_i, trace_taps(), (long long)L);
    int n = 0, C = 0;
    bool done = false;
    auto at = [&](int c, int64_t l) { if (!done && n++ == tap_i) { *C_out = c; *L_out = l; done = true; } };
    auto block = [&](int c, int64_t l) {   // s, h, y of a residual block on [c, l]
        const int64_t lh = plan_sconv(l, cfg.residual_kernel_size, 1, 1).Lout;
        const int64_t ly = plan_sconv(lh, 1, 1, 1).Lout;
        if (done) return;
        at(c, plan_sconv(l, 1, 1, 1).Lout); at(c / cfg.compress, lh);
        if (ly != l && !done) fail(NC_EINVAL, "segment too short: a residual block sees %lld samples", (long long)l);
        at(c, ly);
    };
    const int nf = cfg.n_filters;
    if (!decoder) {
        C = nf; L = plan_sconv(L, cfg.kernel_size, 1, 1).Lout;
        at(C, L);
        for (int i = 0; i < cfg.n_ratios; ++i) {
            const int r = cfg.ratios[cfg.n_ratios - 1 - i];
            block(C, L);
            C *= 2; L = plan_sconv(L, 2 * r, r, 1).Lout;
            at(C, L);
        }
        at(C, L);
        at(cfg.dimension, plan_sconv(L, cfg.last_kernel_size, 1, 1).Lout);
    } else {
        C = nf << cfg.n_ratios; L = plan_sconv(L, cfg.kernel_size, 1, 1).Lout;
        at(C, L); at(C, L);
        for (int i = 0; i < cfg.n_ratios; ++i) {
            const int r = cfg.ratios[i];
            C /= 2; L = L * r;                                   // (L - 1) r + 2r, trimmed by r
            at(C, L);
            block(C, L);
        }
        at(cfg.channels, plan_sconv(L, cfg.last_kernel_size, 1, 1).Lout);
    }
    if (!done) fail(NC_ESTATE, "internal: tap %d not reached", tap_i);
}

const float* EncodecModel::trace_dev(bool decoder, const float* x, int N, int64_t L, int tap_i, const float** stats) {
    if (!loaded) fail(NC_ESTATE, "weights not loaded (call nc_codec_load_weights first)");
    if (!x || N <= 0 || N > GN_MAX_SAMPLES || L <= 0 || L > ((int64_t)1 << 30)) fail(NC_EINVAL, "x, N and L must be given");
    int C = 0; int64_t Lt = 0;
    trace_shape(decoder, L, tap_i, &C, &Lt);
    use_device();
    check_async_errors();
    pool_i = 0;
    struct Off { Trace& t; ~Off() { t.want = -1; } } off{trace};
    trace = Trace{};
    trace.want = tap_i;
    bool hit = false;
    try {
        if (decoder) decoder_stack(x, N, L);
        else encoder_stack(dense_act(x, cfg.channels, L), N);
    } catch (const TapReached&) { hit = true; }
    trace.want = -1;
    const Act& a = trace.act;
    if (!hit || a.C != C || a.L != Lt) fail(NC_ESTATE, "internal: tap %d is [%d, %lld], planned [%d, %lld]", tap_i, a.C, (long long)a.L, C, (long long)Lt);
    if (stats) *stats = a.stats;
    if (trace.lstm && !trace.lstm_has_elu) {   // (NC_LSTM_NO_ELU: the consumer applies the ELU while staging; the tap is defined with it)
        Plan pl; pl.left = 0; pl.right = 0; pl.Lz = a.L; pl.Lp = a.L; pl.Lout = a.L;
        return pad_act(a, nullptr, true, N, pl);
    }
    return materialize(a, N, nullptr, 0);
}

// DecodeFrame on N clips: codes [N,n_q,T'] -> out [N,channels,Lout] dense (x scale[n] when given)
float* EncodecModel::decode_batch(const int64_t* codes, int N, int nq, int64_t Tz, const float* scale, int64_t* Lout) {
    float* emb = alloc((size_t)N * cfg.dimension * Tz);
    launch_emb_sum(book_tab, codes, nq, N, Tz, emb, stream);
    Act o = decoder_stack(emb, N, Tz);
    *Lout = o.L;
    return materialize(o, N, scale, 1);
}

// Consecutive segments with equal `key` run as ONE batch of G*B rows (every operator of the path is per sample: GroupNorm(1,C),
// RMS scale, LSTM state, RVQ), segment-major -- so the batch's codes [G*B, n_q, T'] ARE the G frames' [B, n_q, T'] tensors laid
// end to end, the layout the ABI emits.  Halves the number of dependent LSTM steps of a 2 s clip and doubles every grid.
template <class Body>
void EncodecModel::for_each_group(const std::vector<Seg>& segs, int B, int64_t Seg::*key, Body&& body) {
    static const bool no_overlap = env_flag("NC_ENCODEC_NO_OVERLAP");
    std::vector<std::pair<size_t, int>> runs;   // (first segment, segments) of every group
    std::vector<int> lanes;
    for (size_t f = 0; f < segs.size();) {
        size_t g = f + 1;
        while (g < segs.size() && segs[g].*key == segs[f].*key && (int64_t)(g - f + 1) * B <= 4096) ++g;
        lanes.push_back((!runs.empty() && !no_overlap) ? 1 + (int)((runs.size() - 1) % 2) : 0);   // groups after the first: side streams
        runs.emplace_back(f, (int)(g - f));
        f = g;
    }
    run_batches(lanes, false, [&](size_t i) { body(runs[i].first, runs[i].second); });
}

// The independent batches of one call (the segment groups of a uniform call, the pooled batches of a ragged one), each on its lane.
void EncodecModel::run_batches(const std::vector<int>& lanes, bool lane_pools, const std::function<void(size_t)>& body) {
    hipStream_t const main_stream = stream;
    struct Restore {   // behind every batch, and on an exception
        EncodecModel& m;
        hipStream_t s;
        void operator()() const { m.stream = s; m.on_side_group = false; m.cur_group = 0; m.pool_lane = 0; }
        ~Restore() { (*this)(); }
    } restore{*this, main_stream};
    bool side_used[2] = {false, false};
    NC_HIP(hipEventRecord(ev_fork, main_stream));
    for (size_t i = 0; i < lanes.size(); ++i) {
        const int side = lanes[i] - 1;
        on_side_group = side >= 0;
        cur_group = side + 1;
        if (side >= 0) {
            stream = side_stream[side];
            if (!side_used[side]) NC_HIP(hipStreamWaitEvent(stream, ev_fork, 0));
            side_used[side] = true;
        }
        if (lane_pools) { pool_lane = cur_group; pool_i = 0; }
        body(i);
        restore();
    }
    for (int i = 0; i < 2; ++i)
        if (side_used[i]) {
            NC_HIP(hipEventRecord(ev_join[i], side_stream[i]));
            NC_HIP(hipStreamWaitEvent(main_stream, ev_join[i], 0));
        }
}

void EncodecModel::encode_dev(const float* pcm, int B, int64_t T, int64_t* codes, float* scales, float* emb) {
    if (!loaded) fail(NC_ESTATE, "weights not loaded (call nc_codec_load_weights first)");
    if (!pcm || !codes) fail(NC_EINVAL, "pcm and codes must not be null");
    if (B <= 0 || T <= 0 || T > ((int64_t)1 << 30)) fail(NC_EINVAL, "B and T must be positive");
    use_device();
    check_async_errors();   // an earlier device-pointer call on this handle may have timed out unnoticed
    pool_i = 0;
    const std::vector<Seg> segs = segments(T);
    const int C = cfg.channels, D = cfg.dimension;
    int64_t code_off = 0, emb_off = 0;
    for_each_group(segs, B, &Seg::len, [&](size_t f, int G) {
        const Seg& s = segs[f];
        float* x = alloc((size_t)G * B * C * s.len);
        for (int q = 0; q < G; ++q)   // slice segment f+q out of [B,C,T] into rows [q*B, (q+1)*B) of the dense [G*B,C,len] tensor
            NC_HIP(hipMemcpy2DAsync(x + (size_t)q * B * C * s.len, (size_t)s.len * 4, pcm + segs[f + q].off, (size_t)T * 4, (size_t)s.len * 4,
                                    (size_t)B * C, hipMemcpyDeviceToDevice, stream));
        float* sc = (cfg.normalize && scales) ? scales + (int64_t)f * B : nullptr;
        encode_batch(x, G * B, s.len, s.frames, codes + code_off, sc, emb ? emb + emb_off : nullptr);
        code_off += (int64_t)G * B * n_q * s.frames;
        emb_off += (int64_t)G * B * D * s.frames;
    });
}

// Triangular window + weight sum of the overlap-add (AudioTensorDSP.cs:176-252) on the host: a function of the frame geometry alone --
// computed once per geometry, kept on the device.
void EncodecModel::ola_tables(const std::vector<int64_t>& flen, int64_t stride, int64_t total) {
    const int nfr = (int)flen.size();
    const int64_t L0 = flen[0];
    std::vector<int64_t> key{L0, stride, (int64_t)nfr};
    key.insert(key.end(), flen.begin(), flen.end());
    if (key == ola.key) return;
    std::vector<float> w((size_t)L0), sw((size_t)total, 0.0f);
    for (int64_t i = 0; i < L0; ++i) {
        const float t = (float)((double)(i + 1) / (double)(L0 + 1));
        w[(size_t)i] = 0.5f - std::fabs(t - 0.5f);
    }
    for (int f = 0; f < nfr; ++f)
        for (int64_t i = 0; i < flen[(size_t)f]; ++i) sw[(size_t)(f * stride + i)] = sw[(size_t)(f * stride + i)] + w[(size_t)i];
    float mn = INFINITY;
    for (float v : sw) mn = std::min(mn, v);
    if (mn <= 1e-10f) for (float& v : sw) v = v + 1e-10f;
    NC_HIP(hipStreamSynchronize(stream));   // an earlier call may still read the old tables
    ola.w.reserve((size_t)L0 * 4);
    ola.sw.reserve((size_t)total * 4);
    NC_HIP(hipMemcpy(ola.w.p, w.data(), (size_t)L0 * 4, hipMemcpyHostToDevice));
    NC_HIP(hipMemcpy(ola.sw.p, sw.data(), (size_t)total * 4, hipMemcpyHostToDevice));
    ola.key = key;
}

// Frame pointers / lengths of THIS call: pinned slot -> device arrays ([nfr] pointers, then [nfr] lengths), asynchronously on the stream.
char* EncodecModel::ola_stage(const std::vector<const float*>& fp, const std::vector<int64_t>& flen) {
    const size_t nfr = fp.size(), need = nfr * (sizeof(float*) + sizeof(int64_t));
    if (need > ola.slot_bytes) {
        NC_HIP(hipStreamSynchronize(stream));
        if (ola.pin) NC_HIP(hipHostFree(ola.pin));
        ola.pin = nullptr;
        ola.slot_bytes = std::max<size_t>(1024, 2 * need);
        NC_HIP(hipHostMalloc(&ola.pin, 4 * ola.slot_bytes, hipHostMallocDefault));
        for (bool& u : ola.ev_used) u = false;
    }
    const int slot = ola.next;
    ola.next = (ola.next + 1) & 3;
    if (!ola.ev[slot]) NC_HIP(hipEventCreateWithFlags(&ola.ev[slot], hipEventDisableTiming));
    if (ola.ev_used[slot]) NC_HIP(hipEventSynchronize(ola.ev[slot]));   // the copy that last read this slot (4 calls ago) is done
    char* hs = static_cast<char*>(ola.pin) + (size_t)slot * ola.slot_bytes;
    std::memcpy(hs, fp.data(), nfr * sizeof(float*));
    std::memcpy(hs + nfr * sizeof(float*), flen.data(), nfr * sizeof(int64_t));
    char* dslot = reinterpret_cast<char*>(alloc((need + 3) / 4 + 4));
    NC_HIP(hipMemcpyAsync(dslot, hs, need, hipMemcpyHostToDevice, stream));
    NC_HIP(hipEventRecord(ola.ev[slot], stream));
    ola.ev_used[slot] = true;
    return dslot;
}

void EncodecModel::decode_dev(const int64_t* codes, const float* scales, int B, int64_t T, int nq, float* pcm) {
    if (!loaded) fail(NC_ESTATE, "weights not loaded (call nc_codec_load_weights first)");
    if (!codes || !pcm) fail(NC_EINVAL, "codes and pcm must not be null");
    if (B <= 0 || T <= 0) fail(NC_EINVAL, "No frames provided to decode");                    // Encodec.cs:215-218
    if (nq <= 0 || nq > cfg.n_codebooks) fail(NC_EINVAL, "codes carry %d codebooks; the model has %d", nq, cfg.n_codebooks);
    if (cfg.normalize && !scales) fail(NC_EINVAL, "this model normalises frames: scales must be given");
    use_device();
    check_async_errors();
    pool_i = 0;
    const std::vector<Seg> segs = segments(T);
    const int C = cfg.channels;
    const int nfr = (int)segs.size();
    std::vector<const float*> fp((size_t)nfr);
    std::vector<int64_t> flen((size_t)nfr);
    int64_t code_off = 0;
    for_each_group(segs, B, &Seg::frames, [&](size_t f, int G) {   // equal-length frames decode as one batch
        int64_t Lo = 0;
        const float* out = decode_batch(codes + code_off, G * B, nq, segs[f].frames, cfg.normalize ? scales + (int64_t)f * B : nullptr, &Lo);
        for (int q = 0; q < G; ++q) {
            fp[f + q] = out + (size_t)q * B * C * Lo;
            flen[f + q] = Lo;
        }
        code_off += (int64_t)G * B * nq * segs[f].frames;
    });
    if (cfg.segment_length <= 0) {                                                           // single frame: DecodeFrame output as is
        NC_HIP(hipMemcpyAsync(pcm, fp[0], (size_t)B * C * flen[0] * 4, hipMemcpyDeviceToDevice, stream));
        return;
    }
    const int64_t stride = cfg.segment_stride, total = stride * (nfr - 1) + flen[(size_t)nfr - 1], L0 = flen[0];
    for (int f = 0; f < nfr; ++f)
        if (flen[(size_t)f] > L0) fail(NC_EINVAL, "a later frame is longer than the first one");
    ola_tables(flen, stride, total);
    char* dslot = ola_stage(fp, flen);
    const float** dfp = reinterpret_cast<const float**>(dslot);
    int64_t* dfl = reinterpret_cast<int64_t*>(dslot + (size_t)nfr * sizeof(float*));
    const int64_t n = (int64_t)B * C * total;
    hipLaunchKernelGGL(overlap_add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, dfp, dfl, nfr, L0, ola.w.as<float>(), ola.sw.as<float>(),
                       (int64_t)B * C, stride, total, pcm);
    NC_HIP(hipGetLastError());
}

}  // namespace nc
