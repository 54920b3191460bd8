// DAC FromLatents: continuous projected latents -> codes, raw codebook rows and z.
//
// Reference: Modules/DAC/ResidualVectorQuantizer.cs:243-300 (FromLatents) over VectorQuantizer.cs:99-125 (DecodeLatents) and :62 (OutProj).
// Unlike the encoder's quantizer (stage i + 1 waits for stage i's residual) the codebooks are independent here: codebook i looks at
// channel slice i of the latents and at nothing else.  So ONE launch holds every lookup -- blockIdx.y = codebook, blockIdx.x = a tile
// of 16 frames -- and at 87-150 frames, where a launch of vq_argmin_kernel (nc_rvq.hip) is a handful of workgroups, there are n_q times
// as many.  The out-projection is DacModel::from_codes_dev's: memset z, then out_proj[i] with the RVQ epilogue for i ascending, reading
// slice i of `projected` where it lies.  n_q + 2 launches.
//
// Layout of the lookup: vq_argmin_kernel's.  The codebook sits in LDS transposed ([D][N] and |c|^2: 36 KB for DAC, four workgroups
// per CU), the 64 lanes of a wavefront read 64 consecutive codes of one dimension per ds_read_b32 (conflict-free), each lane scans
// N / 64 codes, and a wavefront min-reduction over (distance, index) picks the winner, lowest index first.  The four frames of a wave go
// through one pass over the codebook, as in dac_rvq_fused_kernel (a code's D LDS words feed four chains).  Arithmetic per (frame, code),
// operation for operation that of vq_argmin_kernel:
//   e2 = fma chain over d ascending of e[d] * e[d], from +0;  cr = fma chain over d ascending of e[d] * c[d], from +0
//   dist = (e2 + |c|^2) - 2 cr;  nc_argmin_scan / nc_argmin_before (nc_math.h): a NaN distance wins, the first one; ties go to the
//   lower index; a row of +inf only gives index 0
// so the codes DAC.encode produced from the same latents come back unchanged.
#include <algorithm>

#include "nc_math.h"
#include "nc_model.h"

namespace nc {

namespace {

constexpr int LL_MAX_D = 16;
constexpr int LL_FW = 4;           // frames per wavefront
constexpr int LL_F = 4 * LL_FW;    // frames per workgroup

struct LatentsLookupArgs {
    const RvqStage* stages;        // device table of the model: cbT / c2 of codebook blockIdx.y
    const float* latents;          // [B][C_lat][.]: channel d of codebook q of frame t of clip b at b * lat_bstride + (q * D + d) * lat_cstride + t
    int64_t lat_bstride, lat_cstride;
    int64_t* codes;                // nullable [B][n_q][.]
    int64_t codes_bstride, codes_cstride;
    float* projected;              // [B][n_q * D][.]
    int64_t proj_bstride, proj_cstride;
    int N, Drt, B;
    int64_t T;                     // frames per clip of this launch
};

// DD > 0: the codebook dimension as a compile-time constant (DAC: 8); with a run-time D every tap of the distance chain is a predicated branch
template <int DD>
__global__ __launch_bounds__(256) void dac_latents_lookup_kernel(const LatentsLookupArgs a) {
    constexpr int MAXD = DD > 0 ? DD : LL_MAX_D;
    const int D = DD > 0 ? DD : a.Drt, N = a.N;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* s_cb = smem;          // [D][N]
    float* s_c2 = smem + D * N;  // [N]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = blockIdx.y;
    const int64_t T = a.T, total = (int64_t)a.B * T;
    const int64_t f0 = (int64_t)blockIdx.x * LL_F + wave * LL_FW;
    // all frames of the wave are fetched before any is searched, and ahead of the codebook copy: one global round trip
    float e[LL_FW][MAXD];
#pragma unroll
    for (int fi = 0; fi < LL_FW; ++fi) {
        const int64_t f = min(f0 + fi, total - 1);
        const int64_t b = f / T, t = f - b * T;
        const float* zp = a.latents + b * a.lat_bstride + (int64_t)q * D * a.lat_cstride + t;
#pragma unroll
        for (int d = 0; d < MAXD; ++d) e[fi][d] = d < D ? zp[(int64_t)d * a.lat_cstride] : 0.0f;
    }
    {   // codebook -> LDS in 16-byte words, 8 reads per thread in flight before their LDS stores; D * N and N are multiples of 4 (host)
        typedef float ll_f32x4 __attribute__((ext_vector_type(4)));
        const RvqStage sg = a.stages[q];
        const ll_f32x4* src = reinterpret_cast<const ll_f32x4*>(sg.cbT);
        ll_f32x4* dst = reinterpret_cast<ll_f32x4*>(s_cb);
        const int nv = D * N / 4;
        for (int i0 = 0; i0 < nv; i0 += 8 * 256) {
            ll_f32x4 r[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) r[u] = src[min(i0 + tid + 256 * u, nv - 1)];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (i0 + tid + 256 * u < nv) dst[i0 + tid + 256 * u] = r[u];
        }
        const ll_f32x4* n4 = reinterpret_cast<const ll_f32x4*>(sg.c2);
        for (int i = tid; i < N / 4; i += 256) reinterpret_cast<ll_f32x4*>(s_c2)[i] = n4[i];
    }
    __syncthreads();
    float e2[LL_FW], best[LL_FW];
    int bi[LL_FW];
#pragma unroll
    for (int fi = 0; fi < LL_FW; ++fi) {
        e2[fi] = 0.0f;
#pragma unroll
        for (int d = 0; d < MAXD; ++d)
            if (d < D) e2[fi] = nc_fma(e[fi][d], e[fi][d], e2[fi]);
        best[fi] = __builtin_inff();
        bi[fi] = 0x7fffffff;
    }
    for (int n = lane; n < N; n += 64) {
        float cv[MAXD];
#pragma unroll
        for (int d = 0; d < MAXD; ++d) cv[d] = d < D ? s_cb[d * N + n] : 0.0f;
        const float cn = s_c2[n];
#pragma unroll
        for (int fi = 0; fi < LL_FW; ++fi) {
            float cr = 0.0f;
#pragma unroll
            for (int d = 0; d < MAXD; ++d)
                if (d < D) cr = nc_fma(e[fi][d], cv[d], cr);
            const float dist = (e2[fi] + cn) - 2.0f * cr;
            if (nc_argmin_scan(dist, best[fi])) { best[fi] = dist; bi[fi] = n; }
        }
    }
    // wavefront min-reduction on (dist, index), lowest index wins ties
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int fi = 0; fi < LL_FW; ++fi) {
            const float od = __shfl_xor(best[fi], off, 64);
            const int oi = __shfl_xor(bi[fi], off, 64);
            if (nc_argmin_before(od, oi, best[fi], bi[fi])) { best[fi] = od; bi[fi] = oi; }
        }
    }
#pragma unroll
    for (int fi = 0; fi < LL_FW; ++fi) {
        const int64_t f = f0 + fi;
        if (f >= total) break;
        if (bi[fi] == 0x7fffffff) bi[fi] = 0;  // a row of +inf only: every distance equal, ATen returns index 0
        const int64_t b = f / T, t = f - b * T;
        if (lane == 0 && a.codes) a.codes[b * a.codes_bstride + (int64_t)q * a.codes_cstride + t] = (int64_t)bi[fi];
        // the raw codebook row (VectorQuantizer.cs:135-142): the codebook is in LDS, transposed -- the same words as cb[bi][lane]
        if (lane < D) a.projected[b * a.proj_bstride + ((int64_t)q * D + lane) * a.proj_cstride + t] = s_cb[lane * N + bi[fi]];
    }
}

}  // namespace

// latents (frames [f0, f0 + n) of rows of pitch T) -> codes (same frames, pitch T; nullable) and projected (dense rows of pitch proj_pitch)
static void launch_latents_lookup(const DacModel& m, int n_q, const float* latents, int C_lat, int64_t T, int64_t f0, int64_t n, int B,
                                  int64_t* codes, float* projected, int64_t proj_pitch, hipStream_t s, Profiler* prof) {
    const int D = m.cfg.codebook_dim, N = m.cfg.codebook_size;
    LatentsLookupArgs a{};
    a.stages = m.rvq_stages.as<RvqStage>();
    a.latents = latents + f0; a.lat_bstride = (int64_t)C_lat * T; a.lat_cstride = T;
    a.codes = codes ? codes + f0 : nullptr; a.codes_bstride = (int64_t)n_q * T; a.codes_cstride = T;
    a.projected = projected; a.proj_bstride = (int64_t)n_q * D * proj_pitch; a.proj_cstride = proj_pitch;
    a.N = N; a.Drt = D; a.B = B; a.T = n;
    const size_t lds = sizeof(float) * ((size_t)D * N + N);
    const int64_t total = (int64_t)B * n;
    const dim3 grid((unsigned)((total + LL_F - 1) / LL_F), (unsigned)n_q);
    if (prof && prof->on) prof->begin(s, NC_KC_RVQ, 3.0 * 2.0 * D * N * (double)total * n_q, 4.0 * total * n_q * (2.0 * D + 2));
    auto launch = [&](auto kern) {
        ensure_dynamic_lds((const void*)kern, 160 * 1024);
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, a);
    };
    if (D == 8) launch(dac_latents_lookup_kernel<8>);
    else launch(dac_latents_lookup_kernel<0>);
    NC_HIP(hipGetLastError());
    if (prof && prof->on) prof->end(s);
}

void DacModel::from_latents_dev(const float* latents, int B, int C_lat, int64_t T, float* z, float* projected, int64_t* codes) {
    const int D = cfg.codebook_dim, N = cfg.codebook_size;
    if (!latents) fail(NC_EINVAL, "latents must not be null");
    if (!z && !projected && !codes) fail(NC_EINVAL, "z, projected and codes are all null: nothing to compute");
    if (B <= 0 || T <= 0) fail(NC_EINVAL, "B and frames must be positive");
    if (C_lat < D) fail(NC_EINVAL, "latents of %d channels hold no codebook of dimension %d", C_lat, D);
    if (T > (int64_t)1 << 30) fail(NC_EINVAL, "too many frames");
    if (!loaded) fail(NC_ESTATE, "weights not loaded (call nc_codec_load_weights first)");
    if (D > LL_MAX_D) fail(NC_EUNSUPPORTED, "codebook_dim %d > %d", D, LL_MAX_D);
    if (N % 4 != 0) fail(NC_EUNSUPPORTED, "codebook of %d entries is not a whole number of 16-byte words", N);
    if (sizeof(float) * ((size_t)D * N + N) > 160 * 1024) fail(NC_EUNSUPPORTED, "codebook of %d x %d does not fit LDS", N, D);
    const int n_q = std::min(cfg.n_codebooks, C_lat / D);   // the codebooks whose cumulative dimension fits (ResidualVectorQuantizer.cs:259-268)
    // The lookup addresses everything in 64 bits.  The out-projection runs on the convolution template, whose row offsets are 32-bit: rows
    // it would refuse are projected piece by piece through dense buffers, on the plan of from_codes (per frame: no halo).
    const ChunkPlan P = z ? chunk_plan(CK_FROM_CODES, B, T) : ChunkPlan{};
    const bool cut = P.n_chunks > 1;
    const int64_t piece = cut ? P.chunk : T;
    if (((int64_t)B * piece + LL_F - 1) / LL_F > 0x7fffffff) fail(NC_EUNSUPPORTED, "%d x %lld frames exceed one launch grid", B, (long long)piece);
    use_device();
    for (int64_t f0 = 0; f0 < T; f0 += piece) {
        const int64_t n = std::min(piece, T - f0);
        const bool own_rows = cut || !projected;   // the raw rows go to the handle's buffer, dense per piece
        if (own_rows) lat.reserve((size_t)B * n_q * D * n * 4);
        float* pj = own_rows ? lat.as<float>() : projected;
        const int64_t pj_pitch = own_rows ? n : T;
        launch_latents_lookup(*this, n_q, latents, C_lat, T, f0, n, B, codes, pj, pj_pitch, stream, &prof);
        if (cut && projected) copy2d(projected + f0, false, (size_t)T * 4, pj, false, (size_t)n * 4, (size_t)n * 4, (size_t)B * n_q * D);
        if (!z) continue;
        if (cut) zq.reserve((size_t)B * latent * n * 4);
        float* zs = cut ? zq.as<float>() : z;
        NC_HIP(hipMemsetAsync(zs, 0, (size_t)B * latent * n * 4, stream));
        for (int i = 0; i < n_q; ++i) {   // from_codes_dev's out-projection, reading slice i of the raw rows where it lies
            ConvIO po{};
            po.x = pj + (int64_t)i * D * pj_pitch; po.x_bstride = (int64_t)n_q * D * pj_pitch; po.x_cstride = pj_pitch; po.x_len = (int32_t)n; po.Tin = n;
            po.y = zs; po.y_bstride = (int64_t)latent * n; po.y_cstride = n;
            po.rvq_zq = zs; po.rvq_res = nullptr; po.epi = EPI_RVQ;
            launch_conv(*out_proj[i], po, B, stream, &prof);
        }
        if (cut) copy2d(z + f0, false, (size_t)T * 4, zs, false, (size_t)n * 4, (size_t)n * 4, (size_t)B * latent);
    }
}

}  // namespace nc
