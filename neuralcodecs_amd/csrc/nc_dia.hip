// Dia's output stage on the device (include/nc_mi355x.h, "Dia output stage"): what Dia.GenerateOutput (Models/Dia.cs:1010-1093) runs between
// the language model's delayed codes [B, T_gen, C] and the waveforms, and ApplyAudioDelay on the way in.
//   revert + cut + mask  BuildRevertIndices / RevertAudioDelay (Modules/Dia/AudioUtils.cs:108-176), Dia.cs:1039-1044
//   decode               item by item at its own length (Dia.cs:1055-1058) == nc_dac_decode_codes_ragged_dev on the packed layout
//   speed                Dia.AdjustSpeed (Dia.cs:947-966) through TorchUtils.Interp (Utils/TorchUtils.cs:58-82)
//   delay                BuildDelayIndices / ApplyAudioDelay (AudioUtils.cs:19-94)
// and its prompt stage ("Dia prompt stage"): what runs between the voice prompts and the language model's delayed prefill.
//   mono mix             Dia.LoadAudio (Dia.cs:851-864) over a packed ragged batch of interleaved prompts
//   encode               prompt by prompt at its own length (Dia.Encode, Dia.cs:988-1001) == nc_dac_encode_ragged_dev on the packed layout
//   prefill              Dia.PrepareAudioPrompt (Dia.cs:329-400): full(-1), BOS row, copy, ApplyAudioDelay -- one closed form, one launch
// and its sampling stage ("Dia sampling stage"): what runs once per frame between the language model's logits and the next row.
//   sample               Dia.DecoderStep from the logits on and SampleNextToken (Dia.cs:530-560, 424-501), binary32, a supplied uniform
//   bookkeeping + write  the EOS countdown of Dia.Generate (Dia.cs:706-746) and DecoderOutput.UpdateOne -- in the same launch
//   collect              the copy into generatedCodes (Dia.cs:786-801): what nc_dia_decode_output_dev takes
// (the host twin of the sampler, nc_dia_sample_host, is csrc/nc_dia_sample_host.hip: written apart from the kernel on purpose)
// The code kernels only move integers; the speed kernel is binary32 with the rounding of every operation written out (__fmul_rn /
// __fadd_rn / __fmaf_rn: the same bits whatever the unit is built with), so every result is a fixed bit pattern.
// The reference's pad masks are dead.  RevertAudioDelay masks `t_idx >= T` AFTER t_idx was clamped to T - 1 (minimum(t + delay, T - 1),
// AudioUtils.cs:121-124), ApplyAudioDelay masks `t - delay[c] >= T` with delay >= 0: neither can fire.  The revert side therefore takes no
// pad argument; the delay side takes one, as ApplyAudioDelay does, and never writes it.
// Tables: none per element.  delay[] and the packed row offsets of up to kDiaItems items travel as kernel arguments; more items are
// more launches.
#include <algorithm>
#include <cmath>

#include "nc_guard.h"
#include "nc_math.h"

namespace nc {

namespace {

constexpr int kDiaMaxC = 32;      // channels (codebooks) of a delay pattern
constexpr int kDiaItems = 32;     // items per launch: their offsets are kernel arguments
constexpr int kDiaTile = 64;      // steps of one [t-tile, C] block of the revert-pack transpose

struct DiaDelay { int32_t d[kDiaMaxC]; };
struct DiaPackItems { int64_t off[kDiaItems], F[kDiaItems]; };             // item k: [C, F] row-major at out + off
struct DiaMixItems { int64_t in_off[kDiaItems], out_off[kDiaItems + 1]; int32_t ch[kDiaItems]; };   // prompt k: [n][ch] at in + in_off -> n frames at out_off[k]
struct DiaSpeedRows { int64_t in_off[kDiaItems], L[kDiaItems], out_off[kDiaItems + 1]; };   // row k: L samples -> out_off[k + 1] - out_off[k]

// ---- kernels ---------------------------------------------------------------------------------------------------------------------
// in [B, T, C] (Dia's layout, C fastest) -> item b0 + blockIdx.y as [C, F] row-major: out[c][t] = in[min(t + delay[c], T - 1)][c], values
// outside [lo, hi] replaced by 0.  A block stages kDiaTile steps x C channels through LDS: the reads run C-fastest over the rows
// t + delay[c] of the tile (every line of that span is used by the block), the writes t-fastest along each output row (8-byte elements,
// consecutive lanes on consecutive addresses: rows may start at any 8-byte offset, nothing wider is stored).
__global__ __launch_bounds__(256) void dia_revert_pack_kernel(const int64_t* __restrict__ in, int b0, int64_t T, int C, DiaDelay dl, DiaPackItems it,
                                                              int64_t lo, int64_t hi, int64_t* __restrict__ out) {
    __shared__ int64_t tile[kDiaMaxC][kDiaTile + 1];
    const int k = blockIdx.y;
    const int64_t F = it.F[k], t0 = (int64_t)blockIdx.x * kDiaTile;
    if (t0 >= F) return;   // the whole block: the grid covers the longest item
    const int nt = (int)(F - t0 < kDiaTile ? F - t0 : kDiaTile);
    const int64_t* __restrict__ src = in + (int64_t)(b0 + k) * T * C;
    for (int e = threadIdx.x; e < nt * C; e += 256) {
        const int t = e / C, c = e - t * C;
        int64_t ti = t0 + t + dl.d[c];
        if (ti > T - 1) ti = T - 1;
        int64_t v = src[ti * C + c];
        if (v < lo || v > hi) v = 0;
        tile[c][t] = v;
    }
    __syncthreads();
    int64_t* __restrict__ dst = out + it.off[k] + t0;
    for (int e = threadIdx.x; e < nt * C; e += 256) {
        const int c = e / nt, t = e - c * nt;
        dst[(int64_t)c * F + t] = tile[c][t];
    }
}

// the same values in Dia's own layout: out [B, Tout, C], one thread per element (C fastest on both sides)
__global__ void dia_revert_delay_kernel(const int64_t* __restrict__ in, int64_t n, int64_t T, int64_t Tout, int C, DiaDelay dl, int64_t lo, int64_t hi,
                                        int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t r = i / C, b = r / Tout, t = r - b * Tout;
    const int c = (int)(i - r * C);
    int64_t ti = t + dl.d[c];
    if (ti > T - 1) ti = T - 1;
    const int64_t v = in[(b * T + ti) * C + c];
    out[i] = (v < lo || v > hi) ? 0 : v;
}

// out[b, t, c] = t - delay[c] < 0 ? bos : in[b, t - delay[c], c]
__global__ void dia_apply_delay_kernel(const int64_t* __restrict__ in, int64_t n, int64_t T, int C, DiaDelay dl, int64_t bos, int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t r = i / C, t = r % T;
    const int c = (int)(i - r * C);
    const int64_t d = dl.d[c];
    out[i] = t - d < 0 ? bos : in[i - d * C];
}

// Rows of packed PCM stretched by linear interpolation, one thread per output sample; a row whose output length equals its input length
// is copied (AdjustSpeed returns its input there).  Position i of T: torch.linspace(0, L - 1, T) in binary32 (step = (end - start) /
// (steps - 1); the first half start + i * step, the second end - (steps - 1 - i) * step; one step: start).  ATen's kernels are built
// with contraction on for every instruction set that has a fused multiply-add, so each position is ONE fused operation there
// (tests/test_dia_output_cpu.py holds this to torch.linspace bit for bit): __fmaf_rn here.  Interp is separate tensor operations, every
// one rounded on its own.  On xp = arange(L): idx = clamp(searchsorted_left(xp, x) - 1, 0, L - 2) = clamp(ceil(x) - 1, ...);
// offset = diff(fp)[idx] (diff(xp) is 1); slope = fp[idx] - offset * xp[idx]; y = offset * x + slope.
__global__ void dia_adjust_speed_kernel(const float* __restrict__ in, int n_rows, DiaSpeedRows rows, float* __restrict__ out) {
    const int64_t o = rows.out_off[0] + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= rows.out_off[n_rows]) return;
    int k = 0;
    while (k + 1 < n_rows && o >= rows.out_off[k + 1]) ++k;
    const int64_t i = o - rows.out_off[k], T = rows.out_off[k + 1] - rows.out_off[k], L = rows.L[k];
    const float* __restrict__ fp = in + rows.in_off[k];
    if (T == L) { out[o] = fp[i]; return; }
    float x = 0.0f;
    if (T > 1) {
        const float end = (float)(L - 1);
        const float step = __fdiv_rn(end, (float)(T - 1));
        x = i < T / 2 ? __fmaf_rn(step, (float)i, 0.0f) : __fmaf_rn(-step, (float)(T - 1 - i), end);
    }
    int64_t idx = (int64_t)ceilf(x) - 1;
    idx = idx < 0 ? 0 : (idx > L - 2 ? L - 2 : idx);
    const float f0 = fp[idx];
    const float offset = __fsub_rn(fp[idx + 1], f0);
    const float slope = __fsub_rn(f0, __fmul_rn(offset, (float)idx));
    out[o] = __fadd_rn(__fmul_rn(offset, x), slope);
}

// The delayed prefill of Dia.PrepareAudioPrompt in closed form (the transpose of dia_revert_pack_kernel): item b0 + blockIdx.y as
// [C, F] row-major at in + off -> out [B, T, C] (C fastest, int32).  With s = t - delay[c]:
//   out[b, t, c] = bos for s <= 0 (row 0 of the prefill and ApplyAudioDelay's BOS mask), codes[c][s - 1] for 1 <= s <= F, -1 behind it.
// The -1 is the torch.full value of Dia.cs:354-358.  ApplyAudioDelay's `pad` is NOT among the arguments: its mask t - delay[c] >= T cannot
// fire (see the head of this file), so the callers take a pad, as the reference does, and nothing ever writes it.
// A block stages kDiaTile steps x C channels through LDS (int32, row stride C | 1 words: odd, so the t-fastest stores of one channel fall on
// distinct banks): the reads run t-fastest along each packed channel row (8-byte elements on consecutive addresses), the writes C-fastest
// over the nt * C consecutive int32 of the tile's rows.  Every step of [0, T) is written by this launch, whatever F: rows behind
// F + delay[c] and items with F = 0 (no prompt) take the fill and the BOS from the same closed form and read nothing.
__global__ __launch_bounds__(256) void dia_prompt_prefill_kernel(const int64_t* __restrict__ in, int b0, int64_t T, int C, DiaDelay dl, DiaPackItems it,
                                                                 int32_t bos, int32_t* __restrict__ out) {
    __shared__ int32_t tile[kDiaTile * (kDiaMaxC + 1)];
    const int k = blockIdx.y, Cs = C | 1;
    const int64_t F = it.F[k], t0 = (int64_t)blockIdx.x * kDiaTile;
    if (t0 >= T) return;   // (the grid is exactly the tiles of T: never taken)
    const int nt = (int)(T - t0 < kDiaTile ? T - t0 : kDiaTile);
    const int64_t* __restrict__ src = in + it.off[k];
    for (int e = threadIdx.x; e < nt * C; e += 256) {
        const int c = e / nt, t = e - c * nt;
        const int64_t s = t0 + t - dl.d[c];
        int32_t v = -1;
        if (s <= 0) v = bos;
        else if (s <= F) v = (int32_t)src[(int64_t)c * F + (s - 1)];   // `prompt.to(torch.int32)`: the low 32 bits
        tile[t * Cs + c] = v;
    }
    __syncthreads();
    int32_t* __restrict__ dst = out + ((int64_t)(b0 + k) * T + t0) * C;
    for (int e = threadIdx.x; e < nt * C; e += 256) {
        const int t = e / C, c = e - t * C;
        dst[e] = tile[t * Cs + c];
    }
}

// Dia.LoadAudio's mono mix (Dia.cs:851-864) over a packed ragged batch, one thread per output frame: prompt k is [n][ch] interleaved at
// in + in_off[k].  The arithmetic of mix_to_mono_kernel (nc_audio.hip) with the rounding written out: a binary32 running sum from 0 in
// channel order, then one division by (float)ch.  A prompt of one channel is copied bit for bit (LoadAudio mixes only for channels > 1).
__global__ void dia_mix_ragged_kernel(const float* __restrict__ in, int n_items, DiaMixItems it, float* __restrict__ out) {
    const int64_t o = it.out_off[0] + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= it.out_off[n_items]) return;
    int k = 0;
    while (k + 1 < n_items && o >= it.out_off[k + 1]) ++k;
    const int ch = it.ch[k];
    const float* __restrict__ x = in + it.in_off[k] + (o - it.out_off[k]) * ch;
    if (ch == 1) { out[o] = x[0]; return; }
    float sum = 0.0f;
    for (int c = 0; c < ch; ++c) sum = __fadd_rn(sum, x[c]);
    out[o] = __fdiv_rn(sum, (float)ch);
}

// ---- sampling stage -------------------------------------------------------------------------------------------------
// Dia.DecoderStep from the logits on (Dia.cs:530-560), SampleNextToken (Dia.cs:424-501), the EOS countdown of Generate (Dia.cs:706-746) and
// DecoderOutput.UpdateOne in one launch.  The definition, step by step, is in include/nc_mi355x.h ("Dia sampling stage").
// One workgroup per item, one wavefront per (item, channel) row (C > kSampleWaves, or a V whose rows do not fit the LDS budget: a wave
// takes every n_waves-th row).  A wave stages its row once into LDS with guidance and masks applied, element v in lane v & 63: every lane
// reads and writes only its own elements afterwards, so nothing a wave does to its row needs a barrier.  Survivors are selected one at a
// time: every lane holds the best of its own elements, a butterfly over the wave finds the best of those by (value descending, index
// ascending), the lane that owned it strikes it out and looks again.  Survivor j lives in lane j.  The sums of steps 7 and 8 are added in
// survivor order by every lane alike (v_readlane of lane j's term): sequential, never a tree.  Plain vector loads and stores, no atomics.
constexpr int kSampleMaxV = 4096, kSampleMaxK = 64, kSampleWaves = 16;
constexpr int kSampleLdsFloats = 15 * 1024;   // rows of all waves: 60 KiB of the 64 KiB a launch gets without asking for more

struct DiaStepArgs {          // the bookkeeping of one generation step; state == nullptr: sampling alone
    int64_t step, max_tokens, maxd, L;
    int32_t apply_mask;
    int64_t* state;
    int32_t* generated;
    int32_t* active_out;
};

__device__ __forceinline__ float lane_f(float x, int j) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), j)); }

// the token of row (b, c), the same in every lane; bad: the row has no token (-1)
__device__ int dia_sample_row(const float* __restrict__ uncond, const float* __restrict__ cond, float* __restrict__ row, int V, int c,
                              const nc_dia_sample_params& p, float u, int lane, bool& bad) {
    const float ninf = -__builtin_inff();
    float bg = ninf;
    int bi = 0x7fffffff;
    bool nan = false;
    for (int v = lane; v < V; v += 64) {
        const float cd = cond[v];
        float g = __fadd_rn(cd, __fmul_rn(p.cfg_scale, __fsub_rn(cd, uncond[v])));
        if (v > p.eos || (c >= 1 && v >= p.eos)) g = ninf;
        else if (v == p.eos) g = __fmul_rn(g, 0.8f);   // (channel 0: the line above took every other channel's)
        row[v] = g;
        nan = nan || g != g;
        if (nc_argmax_before(g, v, bg, bi)) { bg = g; bi = v; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const float og = __shfl_xor(bg, off);
        const int oi = __shfl_xor(bi, off);
        if (nc_argmax_before(og, oi, bg, bi)) { bg = og; bi = oi; }
    }
    bad = false;
    if (p.temperature < 1e-5f) return bi;
    bad = true;
    if (__ballot(nan) != 0) return -1;
    if (bi != p.eos && lane == (p.eos & 63)) row[p.eos] = ninf;
    float lx = ninf;          // the best of this lane's elements: ascending scan, an equal value never replaces the lower index
    int li = 0x7fffffff;
    for (int v = lane; v < V; v += 64) {
        const float x = __fdiv_rn(row[v], p.temperature);
        row[v] = x;
        if (x > lx) { lx = x; li = v; }
    }
    float sx = ninf;          // survivor `lane`
    int si = -1, n = 0;
    for (int j = 0; j < p.top_k; ++j) {
        float bx = lx;
        int bj = li;
        for (int off = 32; off > 0; off >>= 1) {
            const float ox = __shfl_xor(bx, off);
            const int oj = __shfl_xor(bj, off);
            if (ox > bx || (ox == bx && oj < bj)) { bx = ox; bj = oj; }
        }
        if (!(bx > ninf)) break;   // nothing above -inf is left (the same in every lane)
        if (lane == j) { sx = bx; si = bj; }
        n = j + 1;
        if ((bj & 63) == lane) {
            row[bj] = ninf;
            lx = ninf;
            li = 0x7fffffff;
#pragma unroll 8
            for (int v = lane; v < V; v += 64) {
                const float x = row[v];
                if (x > lx) { lx = x; li = v; }
            }
        }
    }
    if (n == 0) return -1;
    const float x0 = lane_f(sx, 0);
    if (x0 == __builtin_inff()) return -1;
    bad = false;
    const float e = lane < n ? nc_expf(__fsub_rn(sx, x0)) : 0.0f;
    unsigned long long keep = n == 64 ? ~0ull : (1ull << n) - 1;
    if (p.top_p < 1.0f) {
        float S = 0.0f;
        for (int j = 0; j < n; ++j) S = __fadd_rn(S, lane_f(e, j));
        const float pj = __fdiv_rn(e, S);
        float cum = 0.0f, before = 0.0f;   // before: c_{lane - 1}
        for (int j = 0; j < n; ++j) {
            if (lane == j) before = cum;
            cum = __fadd_rn(cum, lane_f(pj, j));
        }
        keep = __ballot(lane < n && (lane == 0 || !(before > p.top_p)));
    }
    float S2 = 0.0f;
    for (int j = 0; j < n; ++j)
        if ((keep >> j) & 1) S2 = __fadd_rn(S2, lane_f(e, j));
    const float q = __fdiv_rn(e, S2);
    float d = 0.0f;
    int pick = -1, last = 0;
    for (int j = 0; j < n; ++j) {
        if (!((keep >> j) & 1)) continue;
        d = __fadd_rn(d, lane_f(q, j));
        last = j;
        if (pick < 0 && u < d) pick = j;
    }
    return __builtin_amdgcn_readlane(si, pick < 0 ? last : pick);
}

// grid: one workgroup per item; block: n_waves * 64 threads; dynamic LDS: n_waves rows of Vp floats, then tok[32] and rbad[32]
__global__ __launch_bounds__(kSampleWaves * 64) void dia_sample_kernel(const float* __restrict__ logits, int B, int C, int V, int Vp,
                                                                        nc_dia_sample_params p, const float* __restrict__ uniform, DiaDelay dl,
                                                                        DiaStepArgs st, int64_t* __restrict__ tokens, int32_t* __restrict__ bad) {
    extern __shared__ __attribute__((aligned(16))) float sample_lds[];
    const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    float* row = sample_lds + (size_t)w * Vp;
    int32_t* tok = reinterpret_cast<int32_t*>(sample_lds + (size_t)n_waves * Vp);
    int32_t* rbad = tok + kDiaMaxC;
    for (int c = w; c < C; c += n_waves) {
        const float* uncond = logits + ((int64_t)(2 * b) * C + c) * V;
        bool row_bad;
        const int t = dia_sample_row(uncond, uncond + (int64_t)C * V, row, V, c, p, uniform[(int64_t)b * C + c], lane, row_bad);
        if (lane == 0) {
            tok[c] = t;
            rbad[c] = row_bad;
        }
    }
    __syncthreads();
    if (w != 0) return;
    int any_bad = 0;
    for (int c = 0; c < C; ++c) any_bad |= rbad[c];
    int64_t t = lane < C ? tok[lane] : 0;
    if (!st.state) {
        if (lane < C) tokens[(int64_t)b * C + lane] = t;
        if (lane == 0) bad[b] = any_bad;
        return;
    }
    // lane 0 owns the item's state: it alone reads and writes it; the others take its values
    int64_t det = 0, cdn = 0, fin = 0;
    if (lane == 0) {
        det = st.state[b];
        cdn = st.state[(int64_t)B + b];
        fin = st.state[2 * (int64_t)B + b];
    }
    det = __shfl(det, 0);
    cdn = __shfl(cdn, 0);
    const bool trigger = cdn != 0 && ((det == 0 && tok[0] == p.eos) || st.step >= st.max_tokens - st.maxd);
    if (trigger) det = 1;
    if (trigger && cdn < 0) {
        cdn = st.maxd;
        fin = st.step;
    }
    if (cdn > 0) {
        const int64_t a = st.maxd - cdn, dc = lane < C ? dl.d[lane] : 0;
        if (a == dc) t = p.eos;
        else if (a > dc) t = p.pad;
        cdn -= 1;
    }
    if (lane < C) {
        int32_t* slot = st.generated + ((int64_t)b * st.L + st.step) * C + lane;
        if (!st.apply_mask || *slot == -1) *slot = (int32_t)t;
    }
    if (lane == 0) {
        st.state[b] = det;
        st.state[(int64_t)B + b] = cdn;
        st.state[2 * (int64_t)B + b] = fin;
        st.active_out[b] = cdn != 0;
        bad[b] = bad[b] | any_bad;
    }
}

__global__ void dia_state_init_kernel(int64_t* __restrict__ state, int B) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 3 * B) state[i] = i < B ? 0 : -1;
}

// Dia.cs:786-801: item b0 + blockIdx.y of generated [B, L, C] from its prefill step on -> out [B, T_gen, C], `pad` behind its own length
struct DiaCollectItems { int64_t start[kDiaItems], n[kDiaItems]; };   // item k: rows [start, start + n) of generated, n = length + maxd
__global__ void dia_collect_kernel(const int32_t* __restrict__ generated, int b0, int64_t L, int C, int64_t T_gen, DiaCollectItems it, int64_t pad,
                                   int64_t* __restrict__ out) {
    const int k = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= T_gen * C) return;
    const int64_t t = i / C;
    out[(int64_t)(b0 + k) * T_gen * C + i] = t < it.n[k] ? (int64_t)generated[((int64_t)(b0 + k) * L + it.start[k]) * C + i] : pad;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
unsigned grid_for(int64_t n) {   // as nc_audio.hip
    if (n > (int64_t)0x7fffffff * 256) fail(NC_EINVAL, "too many elements for one launch");
    return (unsigned)((n + 255) / 256);
}

// the delay pattern as a kernel argument; returns max(delay)
int64_t check_delay(int C, const int32_t* delay, DiaDelay& dl) {
    if (!delay) fail(NC_EINVAL, "delay must not be null");
    if (C <= 0 || C > kDiaMaxC) fail(NC_EINVAL, "a delay pattern has 1 to %d channels, not %d", kDiaMaxC, C);
    int64_t maxd = 0;
    dl = DiaDelay{};
    for (int c = 0; c < C; ++c) {
        if (delay[c] < 0) fail(NC_EINVAL, "delay[%d] = %d is negative", c, delay[c]);
        dl.d[c] = delay[c];
        maxd = std::max<int64_t>(maxd, delay[c]);
    }
    return maxd;
}

// `(int)(originalLen / speedFactor)` in binary32 with AdjustSpeed's early returns (Dia.cs:949-959); -1: no such length
int64_t adjust_speed_len(int64_t L, float speed) {
    if (L <= 0 || !std::isfinite(speed) || speed <= 0.0f) return -1;
    if (std::fabs(speed - 1.0f) < 1e-5f) return L;
    const float q = (float)L / speed;
    if (!(q < 2147483648.0f)) return -1;   // the C# cast is undefined from here on
    const int64_t T = (int64_t)(int32_t)q;
    return T <= 0 || T == L ? L : T;
}

// Everything nc_dia_output_query refuses; F_b = lengths[b], the decoded and the adjusted length of every item.
struct DiaOutputPlan {
    DiaDelay dl{};
    int64_t maxd = 0;
    std::vector<int64_t> F, L, T;   // frames, decoded samples, samples after the speed adjustment
    bool stretch = false;           // some row is interpolated
};

DiaOutputPlan plan_output(const DacModel& m, int B, int64_t T_gen, int C, const int32_t* delay, const int64_t* lengths, const float* speed) {
    DiaOutputPlan P;
    if (B <= 0 || !lengths) fail(NC_EINVAL, "B must be positive and lengths must not be null");
    if (C != m.cfg.n_codebooks) fail(NC_EINVAL, "codes of %d channels for a model of %d codebooks", C, m.cfg.n_codebooks);
    P.maxd = check_delay(C, delay, P.dl);
    if (T_gen <= P.maxd) fail(NC_EINVAL, "T_gen = %lld leaves nothing behind a delay of %lld steps", (long long)T_gen, (long long)P.maxd);
    if (T_gen > (int64_t)1 << 40) fail(NC_EINVAL, "T_gen too large");
    P.F.assign(lengths, lengths + B);
    P.L.resize((size_t)B);
    P.T.resize((size_t)B);
    for (int b = 0; b < B; ++b) {
        const int64_t F = lengths[b];
        if (F <= 0 || F > T_gen - P.maxd) fail(NC_EINVAL, "item %d: length %lld is not in [1, T_gen - max(delay) = %lld]", b, (long long)F, (long long)(T_gen - P.maxd));
        const int64_t L = m.decoded_len(F);
        if (L <= 0) fail(NC_EINVAL, "item %d: %lld frames decode to nothing", b, (long long)F);
        int64_t T = L;
        if (speed) {
            if (!std::isfinite(speed[b]) || speed[b] <= 0.0f) fail(NC_EINVAL, "item %d: speed must be finite and positive", b);
            T = adjust_speed_len(L, speed[b]);
            if (T < 0) fail(NC_EINVAL, "item %d: %lld samples at speed %g have no length", b, (long long)L, (double)speed[b]);
            if (T != L && L < 2) fail(NC_EINVAL, "item %d: one sample cannot be interpolated", b);
        }
        P.L[(size_t)b] = L;
        P.T[(size_t)b] = T;
        P.stretch = P.stretch || T != L;
    }
    return P;
}

// the tile counts of launch_revert_pack's grids, refused before anything is launched
void check_pack_grids(int B, const int64_t* F) {
    for (int b = 0; b < B; ++b)
        if ((F[b] + kDiaTile - 1) / kDiaTile > 0x7fffffff) fail(NC_EINVAL, "item %d: too many steps for one launch", b);
}

void launch_revert_pack(const int64_t* in, int B, int64_t T_gen, int C, const DiaDelay& dl, const int64_t* F, int64_t lo, int64_t hi, int64_t* out,
                        hipStream_t s, Profiler* prof) {
    int64_t off = 0;
    for (int b0 = 0; b0 < B; b0 += kDiaItems) {
        const int n = std::min(kDiaItems, B - b0);
        DiaPackItems it{};
        int64_t longest = 0, elems = 0;
        for (int k = 0; k < n; ++k) {
            it.off[k] = off;
            it.F[k] = F[b0 + k];
            off += (int64_t)C * it.F[k];
            elems += (int64_t)C * it.F[k];
            longest = std::max(longest, it.F[k]);
        }
        const int64_t tiles = (longest + kDiaTile - 1) / kDiaTile;
        ProfScope ps(prof, s, NC_KC_ELEM, 0.0, 16.0 * (double)elems);
        hipLaunchKernelGGL(dia_revert_pack_kernel, dim3((unsigned)tiles, (unsigned)n), dim3(256), 0, s, in, b0, T_gen, C, dl, it, lo, hi, out);
        NC_HIP(hipGetLastError());
    }
}

// rows of lengths L[b] -> T[b], both packed; every length is positive and a row with T != L has L >= 2
void launch_adjust_speed(const float* in, int B, const int64_t* L, const int64_t* T, float* out, hipStream_t s, Profiler* prof) {
    int64_t in_off = 0, out_off = 0;
    for (int b0 = 0; b0 < B; b0 += kDiaItems) {
        const int n = std::min(kDiaItems, B - b0);
        DiaSpeedRows rows{};
        rows.out_off[0] = out_off;
        for (int k = 0; k < n; ++k) {
            rows.in_off[k] = in_off;
            rows.L[k] = L[b0 + k];
            in_off += L[b0 + k];
            out_off += T[b0 + k];
            rows.out_off[k + 1] = out_off;
        }
        const int64_t total = out_off - rows.out_off[0];
        ProfScope ps(prof, s, NC_KC_ELEM, 0.0, 12.0 * (double)total);
        hipLaunchKernelGGL(dia_adjust_speed_kernel, dim3(grid_for(total)), dim3(256), 0, s, in, n, rows, out);
        NC_HIP(hipGetLastError());
    }
}

// refuses the output lengths whose launches would not fit a grid (launch_adjust_speed's groups), before anything is launched
void check_speed_grids(int B, const int64_t* T) {
    for (int b0 = 0; b0 < B; b0 += kDiaItems) {
        int64_t total = 0;
        for (int b = b0; b < std::min(B, b0 + kDiaItems); ++b) total += T[b];
        (void)grid_for(total);
    }
}

int64_t sum_of(const std::vector<int64_t>& v) {
    int64_t n = 0;
    for (int64_t x : v) n += x;
    return n;
}

// what a decode call refuses behind plan_output: with both passed, the ragged decode behind the revert finds nothing to refuse
void check_decode_output(const DacModel& m, int B, const DiaOutputPlan& P, int64_t lo, int64_t hi) {
    if (!m.loaded) fail(NC_ESTATE, "weights not loaded (call nc_codec_load_weights first)");
    if (lo < 0 || hi >= m.cfg.codebook_size)
        fail(NC_EINVAL, "valid range [%lld, %lld] lets codes through that a codebook of %d entries does not hold", (long long)lo, (long long)hi, m.cfg.codebook_size);
    check_pack_grids(B, P.F.data());
    if (P.stretch) check_speed_grids(B, P.T.data());
}

// codes_delayed and pcm_packed are device pointers; async on m.stream; the caller has run check_decode_output
void decode_output_dev(nc_codec* h, DacModel& m, const int64_t* codes_delayed, int B, int64_t T_gen, int C, const DiaOutputPlan& P, int64_t lo, int64_t hi,
                       float* pcm_packed) {
    m.use_device();
    m.dia_codes.reserve((size_t)((int64_t)C * sum_of(P.F)) * 8);
    float* decoded = pcm_packed;
    if (P.stretch) {
        m.dia_pcm.reserve((size_t)sum_of(P.L) * 4);
        decoded = m.dia_pcm.as<float>();
    }
    launch_revert_pack(codes_delayed, B, T_gen, C, P.dl, P.F.data(), lo, hi, m.dia_codes.as<int64_t>(), m.stream, &m.prof);
    const nc_status st = nc_dac_decode_codes_ragged_dev(h, m.dia_codes.as<int64_t>(), B, P.F.data(), C, decoded);
    if (st != NC_OK) {
        const std::string msg = get_last_error();
        fail(st, "%s", msg.c_str());
    }
    if (P.stretch) launch_adjust_speed(decoded, B, P.L.data(), P.T.data(), pcm_packed, m.stream, &m.prof);
}

// ---- prompt stage ----------------------------------------------------------------------------------------------------------------
int32_t as_i32(int64_t v, const char* what) {
    if (v < INT32_MIN || v > INT32_MAX) fail(NC_EINVAL, "%s = %lld does not fit the int32 prefill", what, (long long)v);
    return (int32_t)v;
}

// the grid of launch_prefill (the tiles of T_max, the same for every item group) and the size of its output, refused before anything is launched
void check_prefill_grid(int B, int64_t T_max, int C) {
    if (T_max <= 0) fail(NC_EINVAL, "T_max = %lld: with no prompt and no delay nothing holds the BOS row", (long long)T_max);
    if ((T_max + kDiaTile - 1) / kDiaTile > 0x7fffffff || T_max > ((int64_t)1 << 60) / ((int64_t)B * C)) fail(NC_EINVAL, "too many steps for one launch");
}

// packed codes (item b as [C, F[b]], F[b] = 0: no prompt) -> out int32 [B, T_max, C]: one launch per kDiaItems items, each over every step of its items
void launch_prefill(const int64_t* codes, int B, const int64_t* F, int C, const DiaDelay& dl, int32_t bos, int64_t T_max, int32_t* out, hipStream_t s,
                    Profiler* prof) {
    int64_t off = 0;
    const int64_t tiles = (T_max + kDiaTile - 1) / kDiaTile;
    for (int b0 = 0; b0 < B; b0 += kDiaItems) {
        const int n = std::min(kDiaItems, B - b0);
        DiaPackItems it{};
        int64_t elems = 0;
        for (int k = 0; k < n; ++k) {
            it.off[k] = off;
            it.F[k] = F[b0 + k];
            off += (int64_t)C * it.F[k];
            elems += (int64_t)C * it.F[k];
        }
        ProfScope ps(prof, s, NC_KC_ELEM, 0.0, 8.0 * (double)elems + 4.0 * (double)n * (double)T_max * C);
        hipLaunchKernelGGL(dia_prompt_prefill_kernel, dim3((unsigned)tiles, (unsigned)n), dim3(256), 0, s, codes, b0, T_max, C, dl, it, bos, out);
        NC_HIP(hipGetLastError());
    }
}

// the frame totals of launch_mix's groups, refused before anything is launched
void check_mix_grids(int B, const int64_t* n_frames) {
    for (int b0 = 0; b0 < B; b0 += kDiaItems) {
        int64_t total = 0;
        for (int b = b0; b < std::min(B, b0 + kDiaItems); ++b) total += n_frames[b];
        (void)grid_for(total);
    }
}

// prompt b: [n_frames[b]][channels[b]] interleaved, packed -> n_frames[b] mono samples, packed; a group without a frame launches nothing
void launch_mix(const float* in, int B, const int64_t* n_frames, const int32_t* channels, float* out, hipStream_t s, Profiler* prof) {
    int64_t in_off = 0, out_off = 0;
    for (int b0 = 0; b0 < B; b0 += kDiaItems) {
        const int n = std::min(kDiaItems, B - b0);
        DiaMixItems it{};
        it.out_off[0] = out_off;
        const int64_t in0 = in_off;
        for (int k = 0; k < n; ++k) {
            it.in_off[k] = in_off;
            it.ch[k] = channels[b0 + k];
            in_off += n_frames[b0 + k] * channels[b0 + k];
            out_off += n_frames[b0 + k];
            it.out_off[k + 1] = out_off;
        }
        const int64_t total = out_off - it.out_off[0];
        if (total == 0) continue;
        ProfScope ps(prof, s, NC_KC_ELEM, 0.0, 4.0 * (double)(in_off - in0 + total));
        hipLaunchKernelGGL(dia_mix_ragged_kernel, dim3(grid_for(total)), dim3(256), 0, s, in, n, it, out);
        NC_HIP(hipGetLastError());
    }
}

// Everything nc_dia_prompt_query refuses; n[b] samples per channel, F_b the model's frames of them (0: no prompt)
struct DiaPromptPlan {
    DiaDelay dl{};
    int64_t maxd = 0, T_max = 0;
    std::vector<int64_t> n, F;
    std::vector<int32_t> ch;
    bool mix = false;               // some prompt has more than one channel
    int64_t in_samples = 0;         // floats of the packed input
};

DiaPromptPlan plan_prompts(const DacModel& m, int B, int C, const int32_t* delay, const int64_t* lengths, const int32_t* channels) {
    DiaPromptPlan P;
    if (B <= 0 || !lengths) fail(NC_EINVAL, "B must be positive and lengths must not be null");
    if (C != m.cfg.n_codebooks) fail(NC_EINVAL, "a prefill of %d channels for a model of %d codebooks", C, m.cfg.n_codebooks);
    P.maxd = check_delay(C, delay, P.dl);
    P.n.assign(lengths, lengths + B);
    P.F.resize((size_t)B);
    P.ch.assign((size_t)B, 1);
    int64_t maxF = 0;
    for (int b = 0; b < B; ++b) {
        if (lengths[b] < 0) fail(NC_EINVAL, "prompt %d has length %lld", b, (long long)lengths[b]);
        if (lengths[b] > (int64_t)1 << 30) fail(NC_EINVAL, "prompt %d: clip too long", b);   // as nc_dac_encode_ragged
        if (channels) {
            if (channels[b] <= 0) fail(NC_EINVAL, "prompt %d has %d channels", b, channels[b]);
            P.ch[(size_t)b] = channels[b];
            P.mix = P.mix || (channels[b] > 1 && lengths[b] > 0);
        }
        P.F[(size_t)b] = lengths[b] > 0 ? m.frames(lengths[b]) : 0;   // the length rule of nc_dac_ragged_query
        maxF = std::max(maxF, P.F[(size_t)b]);
        P.in_samples += lengths[b] * P.ch[(size_t)b];
    }
    P.T_max = maxF + P.maxd;
    check_prefill_grid(B, P.T_max, C);
    return P;
}

// what an encode call refuses behind plan_prompts: with both passed, nothing behind the first launch finds anything to refuse
void check_encode_prompts(const DacModel& m, int B, const DiaPromptPlan& P, const void* pcm, const void* prefill, int64_t bos, int64_t pad) {
    if (!prefill || (!pcm && P.in_samples > 0)) fail(NC_EINVAL, "nc_dia_encode_prompts: null pointer");
    (void)as_i32(bos, "bos");
    (void)as_i32(pad, "pad");
    if (!m.loaded) fail(NC_ESTATE, "weights not loaded (call nc_codec_load_weights first)");
    if (P.mix) check_mix_grids(B, P.n.data());
}

// pcm_packed and prefill_out are device pointers; async on m.stream; the caller has run check_encode_prompts
void encode_prompts_dev(nc_codec* h, DacModel& m, const float* pcm_packed, int B, int C, const DiaPromptPlan& P, int32_t bos, int32_t* prefill_out) {
    m.use_device();
    const float* mono = pcm_packed;
    if (P.mix) {
        m.dia_pcm.reserve((size_t)sum_of(P.n) * 4);
        launch_mix(pcm_packed, B, P.n.data(), P.ch.data(), m.dia_pcm.as<float>(), m.stream, &m.prof);
        mono = m.dia_pcm.as<float>();
    }
    std::vector<int64_t> lens;   // the prompts that exist: one without samples takes no room in either packed layout
    for (int b = 0; b < B; ++b)
        if (P.n[(size_t)b] > 0) lens.push_back(P.n[(size_t)b]);
    if (!lens.empty()) {
        m.dia_codes.reserve((size_t)((int64_t)C * sum_of(P.F)) * 8);
        const nc_status st = nc_dac_encode_ragged_dev(h, mono, (int32_t)lens.size(), lens.data(), m.cfg.sample_rate, C, m.dia_codes.as<int64_t>());
        if (st != NC_OK) {
            const std::string msg = get_last_error();
            fail(st, "%s", msg.c_str());
        }
    }
    launch_prefill(m.dia_codes.as<int64_t>(), B, P.F.data(), C, P.dl, bos, P.T_max, prefill_out, m.stream, &m.prof);
}

void write_steps(int B, const DiaPromptPlan& P, int32_t* steps_out) {
    if (!steps_out) return;
    for (int b = 0; b < B; ++b) steps_out[b] = (int32_t)(P.F[(size_t)b] + 1);
}

// ---- sampling stage --------------------------------------------------------------------------------------------------------------
// everything nc_dia_sample_dev refuses about the shape and the parameters
void check_sample(int B, int C, int V, const nc_dia_sample_params* p) {
    if (!p) fail(NC_EINVAL, "params must not be null");
    if (B <= 0) fail(NC_EINVAL, "B must be positive");
    if (C < 1 || C > kDiaMaxC) fail(NC_EINVAL, "a row set has 1 to %d channels, not %d", kDiaMaxC, C);
    if (V > kSampleMaxV) fail(NC_EINVAL, "V = %d is above %d", V, kSampleMaxV);
    if (p->eos < 0 || p->eos >= V) fail(NC_EINVAL, "eos = %d is not in [0, V = %d)", p->eos, V);
    if (p->top_k < 1 || p->top_k > kSampleMaxK) fail(NC_EINVAL, "top_k = %d is not in [1, %d]", p->top_k, kSampleMaxK);
    if (!std::isfinite(p->temperature) || !std::isfinite(p->top_p) || !std::isfinite(p->cfg_scale))
        fail(NC_EINVAL, "temperature, top_p and cfg_scale must be finite");
    if (p->temperature < 0.0f) fail(NC_EINVAL, "temperature must not be negative");
    if (p->top_p <= 0.0f) fail(NC_EINVAL, "top_p must be positive");
}

// ONE launch: B workgroups of min(C, 16, what the LDS budget holds) waves
void launch_sample(const float* logits, int B, int C, int V, const nc_dia_sample_params& p, const float* uniform, const DiaDelay& dl, const DiaStepArgs& st,
                   int64_t* tokens, int32_t* bad, hipStream_t s) {
    const int Vp = (V + 3) & ~3;
    const int n_waves = std::min(std::min(C, kSampleWaves), kSampleLdsFloats / Vp);
    const size_t lds = ((size_t)n_waves * Vp + 2 * kDiaMaxC) * 4;
    hipLaunchKernelGGL(dia_sample_kernel, dim3((unsigned)B), dim3((unsigned)n_waves * 64), lds, s, logits, B, C, V, Vp, p, uniform, dl, st, tokens, bad);
    NC_HIP(hipGetLastError());
}

}  // namespace

}  // namespace nc

// ================================================================================================ C ABI
using namespace nc;

extern "C" {

int64_t nc_dia_adjust_speed_len(int64_t L, float speed) { return adjust_speed_len(L, speed); }

nc_status nc_dia_output_query(const nc_codec* h, int32_t B, int64_t T_gen, int32_t C, const int32_t* delay, const int64_t* lengths, const float* speed,
                              int64_t* frames_out, int64_t* decoded_lens, int64_t* out_lens) {
    return guard([&] {
        const DiaOutputPlan P = plan_output(as<DacModel>(h), B, T_gen, C, delay, lengths, speed);
        for (int b = 0; b < B; ++b) {
            if (frames_out) frames_out[b] = P.F[(size_t)b];
            if (decoded_lens) decoded_lens[b] = P.L[(size_t)b];
            if (out_lens) out_lens[b] = P.T[(size_t)b];
        }
    });
}

nc_status nc_dia_decode_output_dev(nc_codec* h, const int64_t* codes_delayed, int32_t B, int64_t T_gen, int32_t C, const int32_t* delay,
                                   const int64_t* lengths, int64_t min_valid, int64_t max_valid, const float* speed, float* pcm_packed) {
    return guard([&] {
        DacModel& m = as<DacModel>(h);
        if (!codes_delayed || !pcm_packed) fail(NC_EINVAL, "nc_dia_decode_output: null pointer");
        const DiaOutputPlan P = plan_output(m, B, T_gen, C, delay, lengths, speed);
        check_decode_output(m, B, P, min_valid, max_valid);
        decode_output_dev(h, m, codes_delayed, B, T_gen, C, P, min_valid, max_valid, pcm_packed);
    });
}

// host pointers: the delayed codes are staged whole, the packed PCM comes back behind the last launch; complete on return
nc_status nc_dia_decode_output(nc_codec* h, const int64_t* codes_delayed, int32_t B, int64_t T_gen, int32_t C, const int32_t* delay,
                               const int64_t* lengths, int64_t min_valid, int64_t max_valid, const float* speed, float* pcm_packed) {
    return guard([&] {
        DacModel& m = as<DacModel>(h);
        if (!codes_delayed || !pcm_packed) fail(NC_EINVAL, "nc_dia_decode_output: null pointer");
        const DiaOutputPlan P = plan_output(m, B, T_gen, C, delay, lengths, speed);
        check_decode_output(m, B, P, min_valid, max_valid);
        OwnStreamScope own(m);
        const size_t n_in = (size_t)((int64_t)B * T_gen * C) * 8, n_out = (size_t)sum_of(P.T) * 4;
        m.rg_in.reserve(n_in);
        m.rg_out.reserve(n_out);
        NC_HIP(hipMemcpyAsync(m.rg_in.p, codes_delayed, n_in, hipMemcpyHostToDevice, m.stream));
        decode_output_dev(h, m, m.rg_in.as<int64_t>(), B, T_gen, C, P, min_valid, max_valid, m.rg_out.as<float>());
        NC_HIP(hipMemcpyAsync(pcm_packed, m.rg_out.p, n_out, hipMemcpyDeviceToHost, m.stream));
        NC_HIP(hipStreamSynchronize(m.stream));
    });
}

nc_status nc_dia_apply_delay_dev(int device_index, const int64_t* codes, int32_t B, int64_t T, int32_t C, const int32_t* delay, int64_t pad, int64_t bos,
                                 int64_t* out, void* hip_stream) {
    return guard([&] {
        (void)pad;   // ApplyAudioDelay's pad mask cannot fire (see the head of this file)
        if (!codes || !out) fail(NC_EINVAL, "null pointer");
        if (B <= 0 || T <= 0) fail(NC_EINVAL, "B and T must be positive");
        DiaDelay dl;
        check_delay(C, delay, dl);
        if (T > (int64_t)1 << 40) fail(NC_EINVAL, "T too large");
        const int64_t n = (int64_t)B * T * C;
        const unsigned grid = grid_for(n);
        use_checked_device(device_index);
        hipLaunchKernelGGL(dia_apply_delay_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(hip_stream), codes, n, T, C, dl, bos, out);
        NC_HIP(hipGetLastError());
    });
}

nc_status nc_dia_revert_delay_dev(int device_index, const int64_t* codes, int32_t B, int64_t T, int32_t C, const int32_t* delay, int64_t min_valid,
                                  int64_t max_valid, int64_t* out, void* hip_stream) {
    return guard([&] {
        if (!codes || !out) fail(NC_EINVAL, "null pointer");
        if (B <= 0) fail(NC_EINVAL, "B must be positive");
        DiaDelay dl;
        const int64_t maxd = check_delay(C, delay, dl);
        if (T <= maxd) fail(NC_EINVAL, "T = %lld leaves nothing behind a delay of %lld steps", (long long)T, (long long)maxd);
        if (T > (int64_t)1 << 40) fail(NC_EINVAL, "T too large");
        const int64_t Tout = T - maxd, n = (int64_t)B * Tout * C;
        const unsigned grid = grid_for(n);
        use_checked_device(device_index);
        hipLaunchKernelGGL(dia_revert_delay_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(hip_stream), codes, n, T, Tout, C, dl, min_valid,
                           max_valid, out);
        NC_HIP(hipGetLastError());
    });
}

nc_status nc_dia_revert_pack_dev(int device_index, const int64_t* codes, int32_t B, int64_t T, int32_t C, const int32_t* delay, const int64_t* lengths,
                                 int64_t min_valid, int64_t max_valid, int64_t* out_packed, void* hip_stream) {
    return guard([&] {
        if (!codes || !out_packed || !lengths) fail(NC_EINVAL, "null pointer");
        if (B <= 0) fail(NC_EINVAL, "B must be positive");
        DiaDelay dl;
        const int64_t maxd = check_delay(C, delay, dl);
        if (T <= maxd) fail(NC_EINVAL, "T = %lld leaves nothing behind a delay of %lld steps", (long long)T, (long long)maxd);
        if (T > (int64_t)1 << 40) fail(NC_EINVAL, "T too large");
        for (int b = 0; b < B; ++b)
            if (lengths[b] <= 0 || lengths[b] > T - maxd)
                fail(NC_EINVAL, "item %d: length %lld is not in [1, T - max(delay) = %lld]", b, (long long)lengths[b], (long long)(T - maxd));
        check_pack_grids(B, lengths);
        use_checked_device(device_index);
        launch_revert_pack(codes, B, T, C, dl, lengths, min_valid, max_valid, out_packed, static_cast<hipStream_t>(hip_stream), nullptr);
    });
}

nc_status nc_dia_adjust_speed_dev(int device_index, const float* pcm_packed, int32_t B, const int64_t* lens, const float* speed, float* out_packed,
                                  void* hip_stream) {
    return guard([&] {
        if (!pcm_packed || !out_packed || !lens || !speed) fail(NC_EINVAL, "null pointer");
        if (B <= 0) fail(NC_EINVAL, "B must be positive");
        std::vector<int64_t> T((size_t)B);
        for (int b = 0; b < B; ++b) {
            if (lens[b] <= 0 || lens[b] > (int64_t)1 << 40) fail(NC_EINVAL, "row %d has length %lld", b, (long long)lens[b]);
            if (!std::isfinite(speed[b]) || speed[b] <= 0.0f) fail(NC_EINVAL, "row %d: speed must be finite and positive", b);
            T[(size_t)b] = adjust_speed_len(lens[b], speed[b]);
            if (T[(size_t)b] < 0) fail(NC_EINVAL, "row %d: %lld samples at speed %g have no length", b, (long long)lens[b], (double)speed[b]);
            if (T[(size_t)b] != lens[b] && lens[b] < 2) fail(NC_EINVAL, "row %d: one sample cannot be interpolated", b);
        }
        check_speed_grids(B, T.data());
        use_checked_device(device_index);
        launch_adjust_speed(pcm_packed, B, lens, T.data(), out_packed, static_cast<hipStream_t>(hip_stream), nullptr);
    });
}

// ---- prompt stage ----------------------------------------------------------------------------------------------------------------
nc_status nc_dia_prompt_query(const nc_codec* h, int32_t B, int32_t C, const int32_t* delay, const int64_t* lengths, int64_t* frames_out, int32_t* steps_out,
                              int64_t* T_max_out) {
    return guard([&] {
        const DiaPromptPlan P = plan_prompts(as<DacModel>(h), B, C, delay, lengths, nullptr);
        for (int b = 0; b < B; ++b)
            if (frames_out) frames_out[b] = P.F[(size_t)b];
        write_steps(B, P, steps_out);
        if (T_max_out) *T_max_out = P.T_max;
    });
}

nc_status nc_dia_encode_prompts_dev(nc_codec* h, const float* pcm_packed, int32_t B, const int64_t* lengths, const int32_t* channels, int32_t C,
                                    const int32_t* delay, int64_t bos, int64_t pad, int32_t* prefill_out, int32_t* steps_out) {
    return guard([&] {
        DacModel& m = as<DacModel>(h);
        const DiaPromptPlan P = plan_prompts(m, B, C, delay, lengths, channels);
        check_encode_prompts(m, B, P, pcm_packed, prefill_out, bos, pad);
        encode_prompts_dev(h, m, pcm_packed, B, C, P, (int32_t)bos, prefill_out);
        write_steps(B, P, steps_out);
    });
}

// host pointers: the packed prompts are staged whole, the prefill comes back behind the last launch; complete on return
nc_status nc_dia_encode_prompts(nc_codec* h, const float* pcm_packed, int32_t B, const int64_t* lengths, const int32_t* channels, int32_t C,
                                const int32_t* delay, int64_t bos, int64_t pad, int32_t* prefill_out, int32_t* steps_out) {
    return guard([&] {
        DacModel& m = as<DacModel>(h);
        const DiaPromptPlan P = plan_prompts(m, B, C, delay, lengths, channels);
        check_encode_prompts(m, B, P, pcm_packed, prefill_out, bos, pad);
        OwnStreamScope own(m);
        const size_t n_in = (size_t)P.in_samples * 4, n_out = (size_t)((int64_t)B * P.T_max * C) * 4;
        m.rg_in.reserve(std::max<size_t>(n_in, 4));
        m.rg_out.reserve(n_out);
        if (n_in) NC_HIP(hipMemcpyAsync(m.rg_in.p, pcm_packed, n_in, hipMemcpyHostToDevice, m.stream));
        encode_prompts_dev(h, m, m.rg_in.as<float>(), B, C, P, (int32_t)bos, m.rg_out.as<int32_t>());
        NC_HIP(hipMemcpyAsync(prefill_out, m.rg_out.p, n_out, hipMemcpyDeviceToHost, m.stream));
        NC_HIP(hipStreamSynchronize(m.stream));
        write_steps(B, P, steps_out);
    });
}

nc_status nc_dia_prefill_pack_dev(int device_index, const int64_t* codes_packed, int32_t B, const int64_t* frames, int32_t C, const int32_t* delay,
                                  int64_t bos, int64_t pad, int64_t T_max, int32_t* out, void* hip_stream) {
    return guard([&] {
        if (!frames || !out) fail(NC_EINVAL, "null pointer");
        if (B <= 0) fail(NC_EINVAL, "B must be positive");
        DiaDelay dl;
        const int64_t maxd = check_delay(C, delay, dl);
        int64_t maxF = 0;
        for (int b = 0; b < B; ++b) {
            if (frames[b] < 0 || frames[b] > (int64_t)1 << 40) fail(NC_EINVAL, "item %d has %lld frames", b, (long long)frames[b]);
            maxF = std::max(maxF, frames[b]);
        }
        if (!codes_packed && maxF > 0) fail(NC_EINVAL, "null pointer");
        const int32_t bos32 = as_i32(bos, "bos");
        (void)as_i32(pad, "pad");   // PrepareAudioPrompt's padValue: taken and never written
        if (T_max < maxF + maxd) fail(NC_EINVAL, "T_max = %lld is below max(frames) + max(delay) = %lld", (long long)T_max, (long long)(maxF + maxd));
        check_prefill_grid(B, T_max, C);
        use_checked_device(device_index);
        launch_prefill(codes_packed, B, frames, C, dl, bos32, T_max, out, static_cast<hipStream_t>(hip_stream), nullptr);
    });
}

nc_status nc_audio_mix_to_mono_ragged_dev(int device_index, const float* in_packed, int32_t B, const int64_t* n_frames, const int32_t* channels,
                                          float* out_packed, void* hip_stream) {
    return guard([&] {
        if (!in_packed || !out_packed || !n_frames || !channels) fail(NC_EINVAL, "null pointer");
        if (B <= 0) fail(NC_EINVAL, "B must be positive");
        for (int b = 0; b < B; ++b) {
            if (n_frames[b] < 0 || n_frames[b] > (int64_t)1 << 40) fail(NC_EINVAL, "prompt %d has %lld frames", b, (long long)n_frames[b]);
            if (channels[b] <= 0) fail(NC_EINVAL, "prompt %d has %d channels", b, channels[b]);
        }
        check_mix_grids(B, n_frames);
        use_checked_device(device_index);
        launch_mix(in_packed, B, n_frames, channels, out_packed, static_cast<hipStream_t>(hip_stream), nullptr);
    });
}

// ---- sampling stage --------------------------------------------------------------------------------------------------------------
nc_status nc_dia_sample_dev(int device_index, const float* logits, int32_t B, int32_t C, int32_t V, const nc_dia_sample_params* params,
                            const float* uniform, int64_t* tokens, int32_t* bad, void* hip_stream) {
    return guard([&] {
        if (!logits || !uniform || !tokens || !bad) fail(NC_EINVAL, "null pointer");
        check_sample(B, C, V, params);
        use_checked_device(device_index);
        launch_sample(logits, B, C, V, *params, uniform, DiaDelay{}, DiaStepArgs{}, tokens, bad, static_cast<hipStream_t>(hip_stream));
    });
}

nc_status nc_dia_generate_state_init_dev(int device_index, int32_t B, int64_t* state, void* hip_stream) {
    return guard([&] {
        if (!state) fail(NC_EINVAL, "null pointer");
        if (B <= 0) fail(NC_EINVAL, "B must be positive");
        use_checked_device(device_index);
        hipLaunchKernelGGL(dia_state_init_kernel, dim3(grid_for(3 * (int64_t)B)), dim3(256), 0, static_cast<hipStream_t>(hip_stream), state, B);
        NC_HIP(hipGetLastError());
    });
}

nc_status nc_dia_generate_step_dev(int device_index, const float* logits, int32_t B, int32_t C, int32_t V, const nc_dia_sample_params* params,
                                   const float* uniform, const int32_t* delay, int64_t step, int64_t max_tokens, int32_t apply_mask, int64_t* state,
                                   int32_t* generated, int64_t L, int32_t* active_out, int32_t* bad, void* hip_stream) {
    return guard([&] {
        if (!logits || !uniform || !state || !generated || !active_out || !bad) fail(NC_EINVAL, "null pointer");
        check_sample(B, C, V, params);
        DiaDelay dl;
        DiaStepArgs st{};
        st.maxd = check_delay(C, delay, dl);
        if (step < 0 || step >= L) fail(NC_EINVAL, "step = %lld is not in [0, L = %lld)", (long long)step, (long long)L);
        if (max_tokens > L) fail(NC_EINVAL, "max_tokens = %lld is above L = %lld", (long long)max_tokens, (long long)L);
        st.step = step;
        st.max_tokens = max_tokens;
        st.L = L;
        st.apply_mask = apply_mask;
        st.state = state;
        st.generated = generated;
        st.active_out = active_out;
        use_checked_device(device_index);
        launch_sample(logits, B, C, V, *params, uniform, dl, st, nullptr, bad, static_cast<hipStream_t>(hip_stream));
    });
}

nc_status nc_dia_generate_lengths(int32_t B, const int64_t* finished, const int32_t* prefill_steps, int64_t final_step, int64_t maxd, int64_t* lengths_out,
                                  int64_t* T_gen_out) {
    return guard([&] {
        if (!finished || !prefill_steps || !lengths_out) fail(NC_EINVAL, "null pointer");
        if (B <= 0 || maxd < 0) fail(NC_EINVAL, "B must be positive and maxd must not be negative");
        int64_t longest = 0;
        for (int b = 0; b < B; ++b) {
            const int64_t f = finished[b] == -1 ? final_step - maxd : finished[b];
            lengths_out[b] = std::max<int64_t>(0, f - prefill_steps[b]);
            longest = std::max(longest, lengths_out[b]);
        }
        if (T_gen_out) *T_gen_out = longest + maxd;
    });
}

nc_status nc_dia_generate_collect_dev(int device_index, const int32_t* generated, int32_t B, int64_t L, int32_t C, const int32_t* prefill_steps,
                                      const int64_t* lengths, int64_t maxd, int64_t pad, int64_t* out, void* hip_stream) {
    return guard([&] {
        if (!generated || !prefill_steps || !lengths || !out) fail(NC_EINVAL, "null pointer");
        if (B <= 0) fail(NC_EINVAL, "B must be positive");
        if (C < 1 || C > kDiaMaxC) fail(NC_EINVAL, "1 to %d channels, not %d", kDiaMaxC, C);
        if (maxd < 0 || maxd > (int64_t)1 << 40 || L <= 0 || L > (int64_t)1 << 40) fail(NC_EINVAL, "maxd and L must fit a code matrix");
        int64_t longest = 0;
        for (int b = 0; b < B; ++b) {
            if (lengths[b] < 0 || prefill_steps[b] < 0) fail(NC_EINVAL, "item %d: negative length or prefill step", b);
            if (lengths[b] > L || prefill_steps[b] + lengths[b] + maxd > L)
                fail(NC_EINVAL, "item %d: steps %lld + %lld + %lld run past L = %lld", b, (long long)prefill_steps[b], (long long)lengths[b], (long long)maxd,
                     (long long)L);
            longest = std::max(longest, lengths[b]);
        }
        const int64_t T_gen = longest + maxd;
        if (T_gen <= 0) fail(NC_EINVAL, "nothing was generated (T_gen = 0)");
        const unsigned grid = grid_for(T_gen * C);
        use_checked_device(device_index);
        for (int b0 = 0; b0 < B; b0 += kDiaItems) {
            const int n = std::min(kDiaItems, B - b0);
            DiaCollectItems it{};
            for (int k = 0; k < n; ++k) {
                it.start[k] = prefill_steps[b0 + k];
                it.n[k] = lengths[b0 + k] + maxd;
            }
            hipLaunchKernelGGL(dia_collect_kernel, dim3(grid, (unsigned)n), dim3(256), 0, static_cast<hipStream_t>(hip_stream), generated, b0, L, C, T_gen, it,
                               pad, out);
            NC_HIP(hipGetLastError());
        }
    });
}

}  // extern "C"
