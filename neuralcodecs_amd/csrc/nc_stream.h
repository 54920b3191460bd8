// Building blocks of the streaming convolution kernels (conv3_stream_kernel, res_a_kernel, down2_kernel, down_stride_kernel, up2_kernel).
//
// The common form.  These layers are thin and long -- on the HBM side of the machine balance -- so the B fragments never touch LDS: a
// workgroup is four waves, wave w owns all rows of its row tile and a span of 32 lanes' worth of columns, and a lane owns a few ADJACENT
// input columns of its channel row (channel 2g on lanes 0-31, 2g + 1 on lanes 32-63: the two kk of a matrix-core step).  Per channel pair
// the lane loads its columns (PF pairs in flight in a register ring), applies the pending GroupNorm (+ add of the second operand) + ELU
// ONCE per element in registers, and builds the taps of its output column(s) from its own values, its lane neighbours' (DPP wavefront
// shifts; one halo load per span covers the first / last lane; reflect or zero padding is an in-lane select) and -- where a step pairs
// taps of the other half's channel -- v_permlane32_swap.  kk = ci*K + k ascending throughout: the canonical chain of DESIGN.md.  Only the
// packed weight image (ConvLayer::build's, shared by the four waves) goes through LDS, double-buffered, one barrier per CB input channels.
// The epilogue adds the bias, forms the GroupNorm block sums of the output in the canonical order (nc_gn.h) with the in-launch finish,
// and stores.
//
// A kernel of the family is therefore: the tile map (nc_xcd_tile_id, nc_frag.h), a prologue (bias -> Ep[], the pending GroupNorm's
// (gamma, beta) -> Gt[], the clip's statistics), its own column geometry and load_pair, the first weight image -> As[0], then per reduction
// block: prefetch of the next image into registers -- its own tap-to-step body (nc_static_for over the channel pairs of the block) -- commit
// to As[cur ^ 1] + barrier; and an epilogue, one column per lane (down2, down_stride) or two (conv3s, resa, up2).  What a new member has
// to think about is the part that differs: which columns a lane loads and which taps it feeds to which matrix-core step.
//
// What is shared here are the pieces that, as force-inlined functions, leave every kernel's instruction stream exactly as the hand-inlined
// text had it: the lane exchanges, the two-input activation and the two-column epilogue of res_a_kernel.  The prologue, the weight double
// buffer and the one-column epilogue were tried as functions too and are NOT here: each of them made the compiler schedule the kernels
// differently (same values, another instruction order and register count), as did the two-column epilogue inside conv3_stream_kernel and
// up2_kernel and nc_in2_act inside up2_kernel -- those kernels keep their own text of these stages.
#pragma once
#include "nc_frag.h"
#include "nc_gn.h"
#include "nc_math.h"

namespace nc {

// lane i <- lane i-1 / lane i+1 of the wavefront (DPP wave_shr:1 / wave_shl:1; the lanes shifted in at the ends are fixed by the caller)
__device__ __forceinline__ float nc_lane_from_left(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float nc_lane_from_right(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130, 0xf, 0xf, false));
}
// the value the same lane of the OTHER half holds
__device__ __forceinline__ float nc_other_half(float v, int hi) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(hi ? r[0] : r[1]);
}
// (even, odd) tap of this lane's channel -> the two B operands of the step pair: b0 = (c0 even | c0 odd), b1 = (c1 even | c1 odd)
__device__ __forceinline__ void nc_step_operands(float even, float odd, float& b0, float& b1) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(even), __float_as_uint(odd), false, false);
    b0 = __uint_as_float(r[0]);   // `even` with its upper half replaced by the lower half of `odd`
    b1 = __uint_as_float(r[1]);   // `odd` with its lower half replaced by the upper half of `even`
}

// ---- activation of a staged value
// the two pending inputs of a layer behind a residual block, g = (gamma_a, beta_a, gamma_b, beta_b) of the channel: GN_a(a) + GN_b(b), then ELU
// (pad_act_kernel's arithmetic: normalise each operand, add, activate)
struct nc_in2_stats { float mu_a, rs_a, mu_b, rs_b; };
__device__ __forceinline__ float nc_in2_act(float va, float vb, float4 g, bool gn, bool elu, nc_in2_stats s) {
    float v = va, w = vb;
    if (gn) {
        v = ((v - s.mu_a) * s.rs_a) * g.x + g.y;
        w = ((w - s.mu_b) * s.rs_b) * g.z + g.w;
    }
    v = v + w;
    return elu ? nc_eluf(v) : v;
}

// ---- two-column epilogue: D[row = (r&3) + 8*(r>>2) + 4*hi] for the lane's two columns col0 + 2*l31 + j.
// GroupNorm block sums of one output (TM row tiles of 32 starting at block row rb0, this wave's 64 columns; colok0 / colok1: the lane's
// columns exist; rows_total: rows of the output from the tile's first) + the in-launch finish; every thread calls it
template <int TM>
__device__ __forceinline__ void nc_stream_gn_out2(const f32x16_t (&acc)[TM][2], const float* Ep, int rows_total, bool colok0, bool colok1, int col0, int l31,
                                                  int hi, int lane, double* gp, int rb0, int nrb, int ncb, unsigned* count, float* stats, unsigned n_wg,
                                                  double n) {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        double a1[2], a2[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float vv[16];
            unsigned okm16 = 0;
            const bool colok = j ? colok1 : colok0;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int R = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                vv[r] = acc[i][j][r] + Ep[R];
                if (colok && R < rows_total) okm16 |= 1u << r;
            }
            nc_gn_slot_sums<false>(vv, okm16, a1[j], a2[j]);
        }
        double s1 = a1[0] + a1[1], s2 = a2[0] + a2[1];
        nc_gn_butterfly_row(s1, s2);
        s1 = nc_gn_swap_add<true>(s1);
        s2 = nc_gn_swap_add<true>(s2);
        const int rbk = rb0 + i, cbk = (col0 >> 5) + (l31 >> 4);
        if ((lane & 47) == 0 && rbk < nrb && cbk < ncb) nc_gn_store_partial(gp + ((int64_t)rbk * ncb + cbk) * 2, s1, s2);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (count != nullptr) nc_gn_arrive_and_finish(gp, count, stats, nrb * ncb, n_wg, n);
}
// bias + 8-byte stores of the lane's two columns; yt: row 4*hi of the tile at the lane's first column
template <int TM>
__device__ __forceinline__ void nc_stream_store2(const f32x16_t (&acc)[TM][2], const float* Ep, int rows_total, float* yt, unsigned cstride, int hi) {
    const int rows_left = rows_total - 4 * hi;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int R = i * 32 + (r & 3) + 8 * (r >> 2);
            if (R >= rows_left) continue;
            const float bias = Ep[R + 4 * hi];
            const f32x2_t v = {acc[i][0][r] + bias, acc[i][1][r] + bias};
            *reinterpret_cast<f32x2_t*>(yt + (size_t)R * cstride) = v;
        }
}

}  // namespace nc
