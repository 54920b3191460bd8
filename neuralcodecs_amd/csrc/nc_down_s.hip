// The second and third down-convolutions of the Encodec 48 kHz encoder in streaming form (SEANetEncoder.cs: [ResnetBlock, ELU, SConv1d(C ->
// 2C, k = 2S, stride S)]; SConv1d.cs:144-173: non-causal reflect pad (S - S/2) + S/2):
//     y = conv_{k2S,sS}( pad( ELU( GN_s(s) + GN_y(y_branch) ) ) )
//   S = 4:  64 -> 128 channels, 24000 -> 6000 steps x 32 clips, 25.2 GFLOP (pad 2 + 2)
//   S = 5: 128 -> 256 channels,  6000 -> 1200 steps x 32 clips, 25.2 GFLOP (pad 3 + 2)
// Until round 6 these layers were a summed / activated copy (pad_act_kernel: 118 us / 57 us) followed by the windowed template on the copy
// (299 us / 404 us on 608 workgroups, 1.2 rounds of the chip): with >= 128 output rows the two-input staging mode re-staged the window per
// row tile and lost.  The streaming form (nc_stream.h) has no window at all: a lane owns S adjacent input columns (S t .. S t +
// S - 1) of its channel row, and the 2S taps of output column t -- x[S t - (S - S/2) .. S t + S + S/2 - 1] -- are the left lane's last
// S - S/2 values, its own S and the right lane's first S/2 (DPP shifts; one halo group of S - S/2 values per 32-column span; reflect as
// in-lane fixes).  kk = ci*2S + k ascending: channel c feeds S matrix-core steps (k even | k odd); with channel c0 on lanes 0-31 and c1 on
// lanes 32-63 ONE v_permlane32_swap(tap 2s, tap 2s+1) per step pair yields both B operands -- its first result is (c0 tap 2s | c0 tap
// 2s+1), its second (c1 tap 2s | c1 tap 2s+1) -- no selects.
//   S = 4: one 16-byte load per operand and channel pair, an 8-byte halo pair.  All 128 output rows in one workgroup (TM = 4, 32 columns
//     per wave), so the activation work is done once.  CB = 8 input channels per barrier = TWO reduction blocks of the packed image
//     ([n_cb][4 channels x 8 taps][128 rows]: the blocks of a row tile lie end to end); one block per barrier -- two channel pairs --
//     measured the same: 315 vs 310 us, the barrier is not what this kernel waits for.
//   S = 5: rows are only 4-byte aligned at that pitch: five dword loads per operand, a halo triple.  The 256 output rows are two row tiles
//     of 128 -- one workgroup each over the same columns, neighbours in the tile map (the second reads the operands out of L2) -- because
//     256 rows x 32 columns of accumulators (128 registers) would leave no room for three waves per SIMD, which this grid needs (2432
//     waves: 1.19 rounds at two per SIMD, one round at three).  Inside a row tile the image's rows are simply kk = c*10 + k, so ANY
//     channel range is contiguous -- four channels (two pairs, 20 KB) per barrier.
// Bit-identical to pad_act_kernel + the windowed launch (NC_NO_DOWN4=1 / NC_NO_DOWN5=1 run those; tests/test_encodec_gpu.py holds both to
// the C oracle).
#include "nc_conv.h"
#include "nc_stream.h"

namespace nc {

template <int N>
struct down_vals {
    float v[N];
    __device__ __forceinline__ float& operator[](int i) { return v[i]; }
    __device__ __forceinline__ float operator[](int i) const { return v[i]; }
};

template <int S>
__global__ __launch_bounds__(256, S == 4 ? 2 : 3) void down_stride_kernel(const Down2Args p) {
    static_assert(S == 4 || S == 5, "the stride-4 and stride-5 layers of the 48 kHz encoder");
    constexpr int TM = 4, BM = 32 * TM, K = 2 * S;
    constexpr int HL = S - S / 2, HR = S / 2;      // halo: the left lane's last HL values, the right lane's first HR
    constexpr bool VEC = S == 4;                   // rows 16-byte aligned at the lane's columns: vector loads
    constexpr bool TILED = S == 5;                 // more than one row tile (Down2Args::n_co_tiles, w_co_stride)
    constexpr int CB = S == 4 ? 8 : 4;             // input channels per barrier
    constexpr int A_FLOATS = CB * K * BM, A_VEC = A_FLOATS / 4, NA = (A_VEC + 255) / 256;
    constexpr int PF = CB / 2;                     // channel pairs in flight (= the pairs of a stage: the ring slot of a pair is its index in the stage)

    __shared__ __attribute__((aligned(16))) float As[2][A_FLOATS];
    __shared__ float Ep[BM];
    __shared__ float4 Gt[128];

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nwg = gridDim.x, bid = blockIdx.x;
    int lin = nc_xcd_tile_id(bid, nwg);
    int co_tile = 0;
    if constexpr (TILED) {
        co_tile = __builtin_amdgcn_readfirstlane(lin % p.n_co_tiles);            // (the row tiles of a column tile are neighbours in the launch order)
        lin /= p.n_co_tiles;
    }
    const int t_tile = __builtin_amdgcn_readfirstlane(lin % p.n_t_tiles);
    const int b = __builtin_amdgcn_readfirstlane(lin / p.n_t_tiles);
    const int T = p.T, Tout = p.Tout, n_cb = p.n_cb, Cin = p.Cin;
    const bool gn_in = p.stats_a != nullptr;
    for (int i = tid; i < BM; i += 256) Ep[i] = p.bias ? p.bias[min(co_tile * BM + i, p.Cout - 1)] : 0.0f;
    float mu_a = 0.0f, rs_a = 1.0f, mu_b = 0.0f, rs_b = 1.0f;
    if (gn_in) {
        mu_a = p.stats_a[2 * b]; rs_a = p.stats_a[2 * b + 1];
        mu_b = p.stats_b[2 * b]; rs_b = p.stats_b[2 * b + 1];
        for (int i = tid; i < n_cb * CB; i += 256) {
            const int c = min(i, Cin - 1);
            Gt[i] = make_float4(p.gamma_a[c], p.beta_a[c], p.gamma_b[c], p.beta_b[c]);
        }
    }
    const nc_in2_stats st = {mu_a, rs_a, mu_b, rs_b};
    const unsigned x_cstride = (unsigned)p.x_cstride;
    const int ocol0 = t_tile * 128 + wave * 32;                    // first OUTPUT column of this wave's span
    const int ocol = ocol0 + l31;
    const int col0 = S * ocol0, col = S * ocol;                    // input columns col .. col + S - 1
    const int colc = min(col, T - S);
    const int hcol = min(max(l31 < 16 ? col0 - HL : col0 + 32 * S, 0), T - HL);   // halo group: left of the span (lanes 0-15) / right of it
    const float* const xa = p.xa + (int64_t)b * p.x_bstride;
    const float* const xb = p.xb + (int64_t)b * p.x_bstride;
    const unsigned x_lane_off = (unsigned)hi * x_cstride + (unsigned)colc;
    const unsigned h_lane_off = (unsigned)hi * x_cstride + (unsigned)hcol;
    const float* wrow = p.w;
    if constexpr (TILED) wrow += (int64_t)co_tile * p.w_co_stride;
    const f32x4_t* const wbase = reinterpret_cast<const f32x4_t*>(wrow);
    const bool first_col = col == 0, last_col = col + S == T;     // reflect: x[-q] = x[q]; x[T + q] = x[T - 2 - q]
    const bool lane_first = l31 == 0, lane_last = l31 == 31;

    f32x16_t acc[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;

    // the lane's S columns and its halo group of one operand row: vectors where they are loaded as such
    using Cols = std::conditional_t<VEC, f32x4_t, down_vals<S>>;
    using Halo = std::conditional_t<VEC, f32x2_t, down_vals<HL>>;
    Cols qa[PF], qb[PF];
    Halo ha[PF], hb[PF];
    const int last_pair = Cin / 2 - 1;
    auto load_pair = [&](int g, Cols& va, Cols& vb, Halo& h_a, Halo& h_b) __attribute__((always_inline)) {
        const size_t ro = (size_t)(2 * min(g, last_pair)) * x_cstride;
        if constexpr (VEC) {
            va = *reinterpret_cast<const f32x4_t*>(xa + ro + x_lane_off);
            vb = *reinterpret_cast<const f32x4_t*>(xb + ro + x_lane_off);
            h_a = *reinterpret_cast<const f32x2_t*>(xa + ro + h_lane_off);
            h_b = *reinterpret_cast<const f32x2_t*>(xb + ro + h_lane_off);
        } else {
#pragma unroll
            for (int i = 0; i < S; ++i) { va[i] = xa[ro + x_lane_off + i]; vb[i] = xb[ro + x_lane_off + i]; }
#pragma unroll
            for (int i = 0; i < HL; ++i) { h_a[i] = xa[ro + h_lane_off + i]; h_b[i] = xb[ro + h_lane_off + i]; }
        }
    };
#pragma unroll
    for (int u = 0; u < PF; ++u) load_pair(u, qa[u], qb[u], ha[u], hb[u]);

    f32x4_t ra[NA];
#pragma unroll
    for (int n = 0; n < NA; ++n) reinterpret_cast<f32x4_t*>(As[0])[tid + 256 * n] = wbase[tid + 256 * n];   // (A_VEC % 256 == 0: every thread, every pass)
    __syncthreads();

    for (int cb = 0; cb < n_cb; ++cb) {
        const int cur = cb & 1;
        const bool more = cb + 1 < n_cb;
        if (more) {
            const f32x4_t* src = wbase + (size_t)(cb + 1) * A_VEC;
#pragma unroll
            for (int n = 0; n < NA; ++n) ra[n] = src[tid + 256 * n];
        }
        const float* Ac = As[cur] + hi * BM + nc_a_lane_off<TM>(l31);
        nc_static_for<CB / 2>([&](auto pt) __attribute__((always_inline)) {
            constexpr int pr = decltype(pt)::value;                 // channel pair within the stage: channels 2 pr (c0), 2 pr + 1 (c1)
            const int g = cb * (CB / 2) + pr;
            const float4 gt = gn_in ? Gt[2 * g + hi] : make_float4(1.0f, 0.0f, 1.0f, 0.0f);
            const Cols va = qa[pr], vb = qb[pr];
            const Halo h_a = ha[pr], h_b = hb[pr];
            load_pair(g + PF, qa[pr], qb[pr], ha[pr], hb[pr]);
            float x[S], h[HL];
#pragma unroll
            for (int i = 0; i < S; ++i) x[i] = nc_in2_act(va[i], vb[i], gt, gn_in, true, st);
#pragma unroll
            for (int i = 0; i < HL; ++i) h[i] = nc_in2_act(h_a[i], h_b[i], gt, gn_in, true, st);
            // taps of output column ocol in order: L[0 .. HL) = x[col - HL ..], the lane's own S values, R[0 .. HR) = x[col + S ..]
            float tap[K];
#pragma unroll
            for (int j = 0; j < HL; ++j) tap[j] = nc_lane_from_left(x[S - HL + j]);
#pragma unroll
            for (int j = 0; j < HR; ++j) tap[HL + S + j] = nc_lane_from_right(x[j]);
#pragma unroll
            for (int j = 0; j < HL; ++j) tap[j] = lane_first ? h[j] : tap[j];
#pragma unroll
            for (int j = 0; j < HR; ++j) tap[HL + S + j] = lane_last ? h[j] : tap[HL + S + j];
#pragma unroll
            for (int j = 0; j < HL; ++j) tap[j] = first_col ? x[HL - j] : tap[j];                       // reflect pad (SConv1d.cs:258-274): x[-q] = x[q]
#pragma unroll
            for (int j = 0; j < HR; ++j) tap[HL + S + j] = last_col ? x[S - 2 - j] : tap[HL + S + j];   //                    x[T + j] = x[T - 2 - j]
#pragma unroll
            for (int i = 0; i < S; ++i) tap[HL + i] = x[i];
            float b0[S], b1[S];
#pragma unroll
            for (int s = 0; s < S; ++s) nc_step_operands(tap[2 * s], tap[2 * s + 1], b0[s], b1[s]);
            // channel c0: kk = 2S (2 pr) + k -> steps 2S pr .. 2S pr + S - 1 of the stage; channel c1: steps 2S pr + S .. 2S pr + 2S - 1
#pragma unroll
            for (int s = 0; s < S; ++s) {
                float fa[TM];
                nc_load_a_frag<TM>(Ac + 2 * (K * pr + s) * BM, l31, fa);
#pragma unroll
                for (int i = 0; i < TM; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], b0[s], acc[i], 0, 0, 0);
            }
#pragma unroll
            for (int s = 0; s < S; ++s) {
                float fa[TM];
                nc_load_a_frag<TM>(Ac + 2 * (K * pr + S + s) * BM, l31, fa);
#pragma unroll
                for (int i = 0; i < TM; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], b1[s], acc[i], 0, 0, 0);
            }
        });
        if (more) {
#pragma unroll
            for (int n = 0; n < NA; ++n) reinterpret_cast<f32x4_t*>(As[cur ^ 1])[tid + 256 * n] = ra[n];
        }
        __syncthreads();
    }

    // ---- epilogue: D[row = (r&3) + 8*(r>>2) + 4*hi][column l31]: one 32x32 block per row tile and wave
    const bool colok = ocol < Tout;
    if (p.gn_part != nullptr) {
        double* const gp = p.gn_part + (int64_t)b * p.gn_nrb * p.gn_ncb * 2;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            float vv[16];
            unsigned okm16 = 0;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int R = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                vv[r] = acc[i][r] + Ep[R];
                if (colok && co_tile * BM + R < p.Cout) okm16 |= 1u << r;
            }
            double s1, s2;
            nc_gn_slot_sums<false>(vv, okm16, s1, s2);
            nc_gn_butterfly(s1, s2);
            const int cbk = ocol0 >> 5;
            const int rbk = co_tile * TM + i;
            if (lane == 0 && rbk < p.gn_nrb && cbk < p.gn_ncb) nc_gn_store_partial(gp + ((int64_t)rbk * p.gn_ncb + cbk) * 2, s1, s2);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (p.gn_count != nullptr)
            nc_gn_arrive_and_finish(gp, p.gn_count + b, p.gn_stats + 2 * b, p.gn_nrb * p.gn_ncb, (unsigned)(TILED ? p.n_t_tiles * p.n_co_tiles : p.n_t_tiles), p.gn_n);
    }
    if (!colok) return;
    float* const yt = p.y + (int64_t)b * p.y_bstride + (unsigned)(co_tile * BM + 4 * hi) * (unsigned)p.y_cstride + (unsigned)ocol;
    const int rows_left = p.Cout - co_tile * BM - 4 * hi;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int R = i * 32 + (r & 3) + 8 * (r >> 2);
            if (R >= rows_left) continue;
            yt[(size_t)R * (unsigned)p.y_cstride] = acc[i][r] + Ep[R + 4 * hi];
        }
}

template <int S>
static bool launch_down_stride(const Down2Args& a, int TM, hipStream_t stream) {
    if (TM != 4) return false;
    hipLaunchKernelGGL(down_stride_kernel<S>, dim3((unsigned)((int64_t)a.B * a.n_t_tiles * (S == 5 ? a.n_co_tiles : 1))), dim3(256), 0, stream, a);
    NC_HIP(hipGetLastError());
    return true;
}
bool launch_down4(const Down2Args& a, int TM, hipStream_t stream) { return launch_down_stride<4>(a, TM, stream); }
bool launch_down5(const Down2Args& a, int TM, hipStream_t stream) { return launch_down_stride<5>(a, TM, stream); }

}  // namespace nc
