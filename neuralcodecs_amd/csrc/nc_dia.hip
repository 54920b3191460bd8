// Dia's output stage on the device (include/nc_mi355x.h, "Dia output stage"): what Dia.GenerateOutput (Models/Dia.cs:1010-1093) runs between
// the language model's delayed codes [B, T_gen, C] and the waveforms, and ApplyAudioDelay on the way in.
//   revert + cut + mask  BuildRevertIndices / RevertAudioDelay (Modules/Dia/AudioUtils.cs:108-176), Dia.cs:1039-1044
//   decode               item by item at its own length (Dia.cs:1055-1058) == nc_dac_decode_codes_ragged_dev on the packed layout
//   speed                Dia.AdjustSpeed (Dia.cs:947-966) through TorchUtils.Interp (Utils/TorchUtils.cs:58-82)
//   delay                BuildDelayIndices / ApplyAudioDelay (AudioUtils.cs:19-94)
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

namespace nc {

namespace {

constexpr int kDiaMaxC = 32;      // channels (codebooks) of a delay pattern
constexpr int kDiaItems = 32;     // items per launch: their offsets are kernel arguments
constexpr int kDiaTile = 64;      // steps of one [t-tile, C] block of the revert-pack transpose

struct DiaDelay { int32_t d[kDiaMaxC]; };
struct DiaPackItems { int64_t off[kDiaItems], F[kDiaItems]; };             // item k: [C, F] row-major at out + off
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

// ---- host side -------------------------------------------------------------------------------------------------------------------
unsigned grid_for(int64_t n) {   // as nc_audio.hip
    if (n > (int64_t)0x7fffffff * 256) fail(NC_EINVAL, "too many elements for one launch");
    return (unsigned)((n + 255) / 256);
}

void set_device(int device_index) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) fail(NC_EDEVICE, "no HIP device available (the engine has no CPU fallback)");
    if (device_index < 0 || device_index >= n) fail(NC_EINVAL, "device index out of range");
    NC_HIP(hipSetDevice(device_index));
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
        set_device(device_index);
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
        set_device(device_index);
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
        set_device(device_index);
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
        set_device(device_index);
        launch_adjust_speed(pcm_packed, B, lens, T.data(), out_packed, static_cast<hipStream_t>(hip_stream), nullptr);
    });
}

}  // extern "C"
