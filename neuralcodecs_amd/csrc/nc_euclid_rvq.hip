// The Euclidean residual vector quantizer of Encodec (ResidualVectorQuantizer.cs:107-157 over EuclideanCodebook.cs:155-182): the
// stage-by-stage search kernel, the all-stages matrix-core kernel, the embedding sum of Decode, their launchers and the op-level test hook.
#include "nc_math.h"
#include "nc_model.h"

namespace nc {

// Euclidean codebook search, D <= 128 (EuclideanCodebook.cs:155-182): per frame dist_n = (|x|^2 + |e_n|^2) - 2*(x.e_n) with fma
// chains over d ascending, argmin with lowest-index ties; then residual -= embed[idx] (ResidualVectorQuantizer.cs:150-152).
// Block = EQ_F frames x 256 threads; thread n scans codes n, n+256, ...; codebook transposed [D][N] streams from L2.
constexpr int EQ_F = 8, EQ_MAXD = EUCLID_MAX_D, EQ_NPT = 4;
__global__ __launch_bounds__(256) void euclid_vq_kernel(float* __restrict__ residual, const float* __restrict__ cbT,
                                                        const float* __restrict__ cb, const float* __restrict__ c2, int N, int D, int B,
                                                        int64_t T, int64_t* __restrict__ codes, int64_t codes_bstride) {
    __shared__ float es[EQ_F][EQ_MAXD];
    __shared__ float e2s[EQ_F];
    __shared__ float bd[EQ_F][4];
    __shared__ int bi[EQ_F][4];
    __shared__ int win[EQ_F];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t f0 = (int64_t)blockIdx.x * EQ_F, total = (int64_t)B * T;
    for (int i = tid; i < EQ_F * D; i += 256) {
        const int f = i / D, d = i - f * D;
        const int64_t fr = f0 + f;
        float v = 0.0f;
        if (fr < total) { const int64_t b = fr / T, t = fr - b * T; v = residual[(b * D + d) * T + t]; }
        es[f][d] = v;
    }
    __syncthreads();
    if (tid < EQ_F) {
        float a = 0.0f;
        for (int d = 0; d < D; ++d) a = nc_fma(es[tid][d], es[tid][d], a);
        e2s[tid] = a;
    }
    __syncthreads();
    float best[EQ_F];
    int besti[EQ_F];
#pragma unroll
    for (int f = 0; f < EQ_F; ++f) { best[f] = __builtin_inff(); besti[f] = 0x7fffffff; }
    for (int n0 = 0; n0 < N; n0 += 256 * EQ_NPT) {
        float cr[EQ_NPT][EQ_F];
#pragma unroll
        for (int u = 0; u < EQ_NPT; ++u)
#pragma unroll
            for (int f = 0; f < EQ_F; ++f) cr[u][f] = 0.0f;
        for (int d = 0; d < D; ++d) {
            float cv[EQ_NPT];
#pragma unroll
            for (int u = 0; u < EQ_NPT; ++u) {
                const int n = n0 + u * 256 + tid;
                cv[u] = n < N ? cbT[(int64_t)d * N + n] : 0.0f;
            }
#pragma unroll
            for (int f = 0; f < EQ_F; ++f) {
                const float ev = es[f][d];
#pragma unroll
                for (int u = 0; u < EQ_NPT; ++u) cr[u][f] = nc_fma(ev, cv[u], cr[u][f]);
            }
        }
#pragma unroll
        for (int u = 0; u < EQ_NPT; ++u) {
            const int n = n0 + u * 256 + tid;
            if (n < N) {
                const float cc = c2[n];
#pragma unroll
                for (int f = 0; f < EQ_F; ++f) {
                    const float dist = (e2s[f] + cc) - 2.0f * cr[u][f];
                    if (nc_argmin_scan(dist, best[f])) { best[f] = dist; besti[f] = n; }
                }
            }
        }
    }
#pragma unroll
    for (int f = 0; f < EQ_F; ++f) {
        float d0 = best[f];
        int i0 = besti[f];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float od = __shfl_xor(d0, off, 64);
            const int oi = __shfl_xor(i0, off, 64);
            if (nc_argmin_before(od, oi, d0, i0)) { d0 = od; i0 = oi; }
        }
        if (lane == 0) { bd[f][wave] = d0; bi[f][wave] = i0; }
    }
    __syncthreads();
    if (tid < EQ_F) {
        float d0 = bd[tid][0];
        int i0 = bi[tid][0];
        for (int w = 1; w < 4; ++w)
            if (nc_argmin_before(bd[tid][w], bi[tid][w], d0, i0)) { d0 = bd[tid][w]; i0 = bi[tid][w]; }
        if (i0 == 0x7fffffff) i0 = 0;
        win[tid] = i0;
        const int64_t fr = f0 + tid;
        if (fr < total) { const int64_t b = fr / T, t = fr - b * T; codes[b * codes_bstride + t] = (int64_t)i0; }
    }
    __syncthreads();
    for (int i = tid; i < EQ_F * D; i += 256) {
        const int f = i / D, d = i - f * D;
        const int64_t fr = f0 + f;
        if (fr < total) {
            const int64_t b = fr / T, t = fr - b * T;
            residual[(b * D + d) * T + t] = es[f][d] - cb[(int64_t)win[f] * D + d];
        }
    }
}

// All n_q stages of the Euclidean RVQ for a block of 32 frames in ONE launch, cross terms on the matrix cores
// (ResidualVectorQuantizer.cs:139-156 over EuclideanCodebook.cs:155-182).  Same arithmetic as euclid_vq_kernel, operation for
// operation: cr_n = fma chain over d ascending from +0 of e_d * c_{n,d} -- which is what a chain of v_mfma_f32_32x32x2_f32 over
// k = d computes for output (row n, column frame) -- then dist_n = (|e|^2 + |c_n|^2) - 2 * cr_n, argmin with the lowest index on
// ties, residual -= embed[idx].  Rows = codes (A fragments straight from the transposed codebook [D][N]: 32 consecutive codes per
// lane half, L2-resident), columns = frames (B fragments from the residual block in LDS, [d][frame]); wave w scans codes
// [w*N/4, (w+1)*N/4) 128 codes at a time (four independent accumulation chains; row l of tile i = code 4 l + i, so a lane's four A
// values per k are one 16-byte load), the reads two groups of steps ahead of the matrix cores.  The residual block never leaves LDS between
// the stages.  8 launches of 63-90 us (600 workgroups re-streaming the 512 KB codebook each) become one of ~0.2 ms on C3.
constexpr int EM_F = 32, EM_MAXD = EUCLID_MAX_D;
typedef float em_f32x16 __attribute__((ext_vector_type(16)));
typedef float em_f32x4 __attribute__((ext_vector_type(4)));
template <int DD>
__global__ __launch_bounds__(256) void euclid_rvq_mfma_kernel(const float* __restrict__ residual, const float* const* __restrict__ cbT_ptrs,
                                                              const float* const* __restrict__ cb_ptrs, const float* const* __restrict__ c2_ptrs,
                                                              int n_q, int N, int B, int64_t T, int64_t* __restrict__ codes,
                                                              int64_t codes_bstride) {
    constexpr int D = DD;
    constexpr int NWV = 4;   // wavefronts that share a stage's codebook scan, N / NWV codes each
    __shared__ float es[EM_MAXD][EM_F + 1];   // residual block [d][frame]: lane (frame, k half) of a B fragment reads es[2kp + half][frame]; rows padded by one
                                              // word -- the residual update walks d across the lanes (unpadded: every lane of a wave on ONE bank)
    __shared__ float e2s[EM_F];
    __shared__ __attribute__((aligned(16))) float c2s[1024];   // |c_n|^2 of the stage (N <= 1024: the launcher routes larger codebooks to euclid_vq_kernel)
    __shared__ float bd[NWV][EM_F];
    __shared__ int bi[NWV][EM_F];
    __shared__ int win[EM_F];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    const int64_t f0 = (int64_t)blockIdx.x * EM_F, total = (int64_t)B * T;
    for (int i = tid; i < EM_F * D; i += 64 * NWV) {
        const int d = i >> 5, f = i & 31;
        const int64_t fr = f0 + f;
        float v = 0.0f;
        if (fr < total) { const int64_t b = fr / T, t = fr - b * T; v = residual[(b * D + d) * T + t]; }
        es[d][f] = v;
    }
    const int npw = N / NWV;                 // codes per wave (a multiple of 128)
    const int npass = npw / 128;
    // (the stage's pointers come out of a pointer table: say that they are global memory, or the reads are issued as flat loads, which
    // count against the LDS counter too and serialise with the B-fragment reads)
    typedef __attribute__((address_space(1))) const em_f32x4* em_gp4;
    typedef __attribute__((address_space(1))) const float* em_gp1;
    // 128 codes per pass as four row tiles; row l of tile i is code n0 + 4 l + i, so the four A values a lane needs for one k are four
    // consecutive codes of the transposed codebook: ONE 16-byte load, 512 contiguous bytes per lane half.  The reads run two groups of
    // G matrix-core steps ahead through a ring of FOUR register sets (a pass is 8 groups: every pass starts on set 0, so the ring runs
    // on across the passes AND the stages -- the first two groups of the next pass / the next stage's first pass are in flight under the
    // last two groups of this one, the argmin, the hand-off and the residual update; filled per pass, every pass and every stage began
    // with an exposed L2 round trip: 288 -> 251 us on C3's 150-workgroup grid together with the two changes below)
    constexpr int G = 8, NG = DD / 2 / G;    // matrix-core steps per group, groups per pass
    static_assert(NG % 4 == 0, "the four-set ring must start every pass on set 0");
    const int64_t kstride = (int64_t)2 * N / 4;                            // float4 words per MFMA step (two codebook rows)
    auto pass_ptr = [&](int q, int pass) __attribute__((always_inline)) -> em_gp4 {
        return (em_gp4)(cbT_ptrs[q] + (int64_t)hi * N + wave * npw + pass * 128 + 4 * l31);   // k = hi at kp = 0
    };
    em_f32x4 av[4][G];
    em_gp4 ap = pass_ptr(0, 0);
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int u = 0; u < G; ++u) av[g][u] = ap[(int64_t)(g * G + u) * kstride];
    // |c_n|^2 of a stage: in registers one stage ahead, in LDS for the stage's scans (the argmin read them from global memory per pass)
    constexpr int C2R = 1024 / (64 * NWV);
    float c2r[C2R];
#pragma unroll
    for (int i = 0; i < C2R; ++i) c2r[i] = ((em_gp1)c2_ptrs[0])[min(tid + i * 64 * NWV, N - 1)];
    for (int q = 0; q < n_q; ++q) {
        const float* __restrict__ cb = cb_ptrs[q];
        __syncthreads();                     // es holds the residual entering this stage
#pragma unroll
        for (int i = 0; i < C2R; ++i)
            if (tid + i * 64 * NWV < N) c2s[tid + i * 64 * NWV] = c2r[i];
        if (q + 1 < n_q) {
#pragma unroll
            for (int i = 0; i < C2R; ++i) c2r[i] = ((em_gp1)c2_ptrs[q + 1])[min(tid + i * 64 * NWV, N - 1)];
        }
        if (tid < EM_F) {
            float a = 0.0f;
            // |e|^2: ONE fma chain over d ascending (the canonical order), the LDS reads 16 at a time ahead of their 16 dependent fmas
            // (rolled, every fma waited for its own read: 2.0 us of a 27 us stage)
#pragma unroll 1
            for (int d0 = 0; d0 < D; d0 += 16) {
                float ev[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) ev[u] = es[d0 + u][tid];
#pragma unroll
                for (int u = 0; u < 16; ++u) a = nc_fma(ev[u], ev[u], a);
            }
            e2s[tid] = a;
        }
        __syncthreads();
        const float e2 = e2s[l31];
        float best = __builtin_inff();
        int besti = 0x7fffffff;
        for (int pass = 0; pass < npass; ++pass) {
            const int n0 = wave * npw + pass * 128;
            const bool last_pass = pass + 1 == npass;
            const bool has_next = !last_pass || q + 1 < n_q;
            const em_gp4 ap_next = last_pass ? pass_ptr(min(q + 1, n_q - 1), 0) : ap + 32;   // (+ 128 codes)
            em_f32x16 acc[4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                if (g + 2 < NG) {
#pragma unroll
                    for (int u = 0; u < G; ++u) av[(g + 2) % 4][u] = ap[(int64_t)((g + 2) * G + u) * kstride];
                } else if (has_next) {
#pragma unroll
                    for (int u = 0; u < G; ++u) av[(g + 2) % 4][u] = ap_next[(int64_t)((g + 2 - NG) * G + u) * kstride];
                }
                __builtin_amdgcn_sched_barrier(0);   // the reads of group g+2 stay ahead of the matrix-core steps of group g
#pragma unroll
                for (int u = 0; u < G; ++u) {
                    const float bv = es[2 * (g * G + u) + hi][l31];
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[g % 4][u][i], bv, acc[i], 0, 0, 0);
                }
            }
            ap = ap_next;
            // D[row = (r & 3) + 8 (r >> 2) + 4 hi][column = l31].  A lane meets its codes in ASCENDING order (code = n0 + 4 row + i: rows ascend with r,
            // i is the inner loop, n0 ascends over the passes), so the ascending-scan form of ATen's order applies: an equal distance never
            // replaces the incumbent, a NaN takes over once.  (The lane halves and the waves are merged with the any-order form below.)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int nb = n0 + 4 * ((r & 3) + 8 * (r >> 2) + 4 * hi);
                const em_f32x4 cc = *reinterpret_cast<const em_f32x4*>(c2s + nb);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float dist = (e2 + cc[i]) - 2.0f * acc[i][r];
                    if (nc_argmin_scan(dist, best)) { best = dist; besti = nb + i; }
                }
            }
        }
        {   // the two lane halves hold the same frame; then the four waves meet in LDS
            const float od = __shfl_xor(best, 32, 64);
            const int oi = __shfl_xor(besti, 32, 64);
            if (nc_argmin_before(od, oi, best, besti)) { best = od; besti = oi; }
            if (hi == 0) { bd[wave][l31] = best; bi[wave][l31] = besti; }
        }
        __syncthreads();
        if (tid < EM_F) {
            float d0 = bd[0][tid];
            int i0 = bi[0][tid];
            for (int w = 1; w < NWV; ++w)
                if (nc_argmin_before(bd[w][tid], bi[w][tid], d0, i0)) { d0 = bd[w][tid]; i0 = bi[w][tid]; }
            if (i0 == 0x7fffffff) i0 = 0;
            win[tid] = i0;
            const int64_t fr = f0 + tid;
            if (fr < total) { const int64_t b = fr / T, t = fr - b * T; codes[b * codes_bstride + (int64_t)q * T + t] = (int64_t)i0; }
        }
        __syncthreads();
        {   // residual -= embed[idx]: thread (d = tid % D, frames f = tid / D + (64 NWV / D) u) -- a frame's code vector is one coalesced 512-byte
            // read; all of a thread's reads are issued before the first is used (one L2 round trip per stage instead of one per element)
            constexpr int FS = 64 * NWV / D, NU = EM_F / FS;
            static_assert((64 * NWV) % D == 0 && EM_F % FS == 0, "update map");
            const int d = tid % D, fb = tid / D;
            float cv[NU];
#pragma unroll
            for (int u = 0; u < NU; ++u) cv[u] = ((em_gp1)cb)[(int64_t)win[fb + FS * u] * D + d];
#pragma unroll
            for (int u = 0; u < NU; ++u) es[d][fb + FS * u] = es[d][fb + FS * u] - cv[u];
        }
    }
}

// ResidualVectorQuantizer.Decode (:107-124): emb = ((0 + e_0[idx_0]) + e_1[idx_1]) + ...
__global__ void emb_sum_kernel(const int64_t* __restrict__ codes, const float* const* __restrict__ cbs, int n_q, int N, int D, int B,
                               int64_t T, float* __restrict__ emb) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * D * T) return;
    const int64_t t = i % T, r = i / T;
    const int d = (int)(r % D);
    const int64_t b = r / D;
    float a = 0.0f;
    for (int q = 0; q < n_q; ++q) {
        int64_t c = codes[(b * n_q + q) * T + t];
        if (c < 0) c = 0;
        if (c >= N) c = N - 1;
        a = a + cbs[q][c * D + d];
    }
    emb[i] = a;
}

// ---------------------------------------------------------------------------------------------- launchers
void EuclidBooks::add(const Codebook& b) {
    N = b.N; D = b.D;
    cb.push_back(b.cb.as<float>()); cbT.push_back(b.cbT.as<float>()); c2.push_back(b.c2.as<float>());
}
void EuclidBooks::upload() {
    const size_t n = cb.size() * sizeof(float*);
    d_cb.reserve(n); d_cbT.reserve(n); d_c2.reserve(n);
    NC_HIP(hipMemcpy(d_cb.p, cb.data(), n, hipMemcpyHostToDevice));
    NC_HIP(hipMemcpy(d_cbT.p, cbT.data(), n, hipMemcpyHostToDevice));
    NC_HIP(hipMemcpy(d_c2.p, c2.data(), n, hipMemcpyHostToDevice));
}

void launch_euclid_rvq(const EuclidBooks& bk, int n_q, int form, float* residual, int B, int64_t T, int64_t* codes, hipStream_t s) {
    static const bool no_mfma_vq = env_present("NC_EUCLID_NO_MFMA");
    const int N = bk.N, D = bk.D;
    const bool fits = N % 512 == 0 && N <= 1024 && D == 128;
    if (form == 1 && !fits) fail(NC_EUNSUPPORTED, "the matrix-core Euclidean RVQ takes D == 128 and N = 512 or 1024");
    const int64_t total = (int64_t)B * T;
    if (form == 1 || (form < 0 && !no_mfma_vq && fits)) {
        // all stages in one launch, cross terms on the matrix cores (the residual block stays in LDS between the stages)
        hipLaunchKernelGGL(euclid_rvq_mfma_kernel<128>, dim3((unsigned)((total + EM_F - 1) / EM_F)), dim3(256), 0, s, residual,
                           bk.d_cbT.as<const float*>(), bk.d_cb.as<const float*>(), bk.d_c2.as<const float*>(), n_q, N, B, T, codes,
                           (int64_t)n_q * T);
    } else {
        for (int q = 0; q < n_q; ++q)
            hipLaunchKernelGGL(euclid_vq_kernel, dim3((unsigned)((total + EQ_F - 1) / EQ_F)), dim3(256), 0, s, residual, bk.cbT[(size_t)q],
                               bk.cb[(size_t)q], bk.c2[(size_t)q], N, D, B, T, codes + (int64_t)q * T, (int64_t)n_q * T);
    }
    NC_HIP(hipGetLastError());
}

void launch_emb_sum(const EuclidBooks& bk, const int64_t* codes, int n_q, int B, int64_t T, float* emb, hipStream_t s) {
    const int64_t n = (int64_t)B * bk.D * T;
    hipLaunchKernelGGL(emb_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, codes, bk.d_cb.as<const float*>(), n_q, bk.N, bk.D, B, T, emb);
    NC_HIP(hipGetLastError());
}

void op_euclid_rvq(const float* residual_in, int B, int D, int64_t T, const float* books_host, int n_q, int N, int form, int64_t* codes_host, float* residual_out) {
    std::vector<Codebook> books((size_t)n_q);
    EuclidBooks bk;
    for (int q = 0; q < n_q; ++q) {
        books[(size_t)q].build(books_host + (int64_t)q * N * D, N, D);
        bk.add(books[(size_t)q]);
    }
    bk.upload();
    DevBuf res, codes;
    const size_t nb = (size_t)B * D * T * 4;
    res.reserve(nb); codes.reserve((size_t)B * n_q * T * 8);
    NC_HIP(hipMemcpy(res.p, residual_in, nb, hipMemcpyHostToDevice));
    launch_euclid_rvq(bk, n_q, form == 1 ? 1 : 0, res.as<float>(), B, T, codes.as<int64_t>(), nullptr);
    NC_HIP(hipDeviceSynchronize());
    NC_HIP(hipMemcpy(codes_host, codes.p, (size_t)B * n_q * T * 8, hipMemcpyDeviceToHost));
    if (residual_out) NC_HIP(hipMemcpy(residual_out, res.p, nb, hipMemcpyDeviceToHost));
}

}  // namespace nc
