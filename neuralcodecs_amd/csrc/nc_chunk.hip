// Halo derivation, the chunk planner, and DAC / SNAC Encode / Decode / FromCodes run window by window: long clips in several windows,
// and every host-pointer call (a clip that is not cut is one window, the ck_* buffers are its staging).
//
// DAC and SNAC are convolutional with a finite receptive field (SNAC's attention is local to non-overlapping windows), so a clip can be
// cut along the frame axis: chunk j keeps frames [f0, f1) and runs the EXISTING launch sequence on the window
// [f0 - halo_l, f1 + halo_r) clipped to the clip.  A window edge that is a true clip edge gets the layers' own edge handling (zero
// padding, the right zero-pad to the hop multiple through x_len < Tin); an interior window edge is wrong only inside the halo, which
// is dropped.  Every conv instance computes a column from the same operands in the same order wherever the column sits in its tile
// (what the bit-exactness against the C oracle and the batch-invariance tests rest on), so chunked == one-shot bit for bit.
//
// Windows are gathered into dense buffers (ck_*) and the kept columns scattered into the caller's full-length arrays by pitched copies
// on the handle's stream, so the activation arena and every workspace are sized by the window, not the clip.
//
// ---- halo derivation (closed form from the layer table) ------------------------------------------------------------------------------
// Notation: a stage at cumulative stride S (S samples of that stage per latent frame).  For the ENCODER let frame F depend on the
// stage's samples [F*S - l, F*S + r].  Walking from the latent back to the PCM:
//     final conv (DAC k3 pad 1: l = r = 1; SNAC k7 pad 3: l = r = 3)
//     SNAC LocalMHA at frame rate: a frame depends on every frame of its window, and a window sits anywhere relative to the frame:
//         l += W - 1, r += W - 1           (a contaminated frame contaminates its whole window)
//     per block, last block first:  down conv k = 2s, stride s, pad p = ceil(s/2): out[t] reads in[t*s - p .. t*s - p + 2s - 1]
//         l = l*s + p,  r = r*s + (2s - 1 - p),  S *= s
//       then its three k7 units at dilation 1, 3, 9 (dense or depthwise, pad 3d): l += 3*(1+3+9) = 39, r += 39   (the 1x1 adds none)
//     stem k7: l += 3, r += 3
// With S = hop: a change of sample x (frame fx = x / hop) moves frames fx - ceil(r/hop) .. fx + ceil(l/hop):
//     enc_left = ceil(r / hop), enc_right = ceil(l / hop)
// SNAC's quantiser pools aligned blocks of vq_stride frames (avg_pool1d / repeat_interleave), so codes and zq of a whole block move
// with any of its frames: + (max vq_stride - 1) on both sides.
// For the DECODER let frame f influence the stage's samples [f*S - a, f*S + b].  Walking forward:
//     first conv k7 at frame rate (SNAC: depthwise k7 + 1x1): a = b = 3;  SNAC LocalMHA: a += W - 1, b += W - 1
//     per block: transposed conv k = 2s, stride s, pad p: in[i] writes out[i*s - p .. i*s - p + 2s - 1]
//         a = a*s + p,  b = b*s + (2s - 1 - p),  S *= s;   NoiseBlock is per sample;   three units: a += 39, b += 39
//     head k7: a += 3, b += 3
//     dec_left = ceil(a / hop), dec_right = ceil(b / hop)   (in frames of hop output samples)
// The reach only grows towards the sample side (l*s + p >= l*s), so the last stage is the binding one for every stage: a window whose
// latent frames keep clear of an interior edge by the halo keeps every intermediate stage's dependency cone inside the window too.
// align = lcm(vq_strides[0], attn_window) for SNAC (the lcm SNAC.Preprocess pads to), 1 for DAC; chunk boundaries are multiples of it
// (whole attention windows and whole pooling blocks per window) and every halo is rounded up to it.
// A chunk needs on its LEFT what a change reaches to its RIGHT: halo_left = *_right, halo_right = *_left.
#include <algorithm>

#include "nc_guard.h"
#include "nc_limits.h"
#include "nc_pool.h"

namespace nc {

namespace {

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

void halo_from_layers(const int32_t* er, int ne, const int32_t* dr, int nd, int final_reach, int W, int vq_max, int64_t align, nc_halo* out) {
    if (ne <= 0 || ne > 8 || nd <= 0 || nd > 8) fail(NC_EINVAL, "encoder/decoder rate lists must hold 1..8 entries");
    int64_t l = final_reach, r = final_reach, hop = 1;
    if (W > 1) { l += W - 1; r += W - 1; }
    for (int i = ne - 1; i >= 0; --i) {
        const int64_t s = er[i], p = (s + 1) / 2;
        if (s <= 0) fail(NC_EINVAL, "encoder rate must be positive");
        l = l * s + p; r = r * s + (2 * s - 1 - p);
        l += 39; r += 39;
        hop *= s;
    }
    l += 3; r += 3;
    int64_t a = 3, b = 3, H = 1;
    if (W > 1) { a += W - 1; b += W - 1; }
    for (int i = 0; i < nd; ++i) {
        const int64_t s = dr[i], p = (s + 1) / 2;
        if (s <= 0) fail(NC_EINVAL, "decoder rate must be positive");
        a = a * s + p; b = b * s + (2 * s - 1 - p);
        a += 39; b += 39;
        H *= s;
    }
    a += 3; b += 3;
    out->align = align;
    out->enc_left = round_up(ceil_div(r, hop) + (vq_max - 1), align);
    out->enc_right = round_up(ceil_div(l, hop) + (vq_max - 1), align);
    out->dec_left = round_up(ceil_div(a, H), align);
    out->dec_right = round_up(ceil_div(b, H), align);
}

int64_t pitch16(int64_t L) { return L >= 256 ? ((L + 15) & ~(int64_t)15) : L; }   // upper bound of nc_dac.hip's row pitch

// the built-in chunk of NC_CHUNK_AUTO: long enough that the recomputed halo stays near a tenth of the work
int64_t auto_chunk(const nc_halo& h, bool decode) {
    const int64_t hmax = decode ? std::max(h.dec_left, h.dec_right) : std::max(h.enc_left, h.enc_right);
    return round_up(std::max<int64_t>(1024, 16 * hmax), h.align);
}

// Would launch_conv refuse a layer of the one-shot call?  The same two inequalities (nc_limits.h), asked of every stage of the layer
// table with the largest row tile the template has (bm = 512 bounds every instance) and every up-conv taken as the multiply-shift
// sub-pixel form: conservative, never permissive.
bool oneshot_fits(const int32_t* er, int ne, int enc_dim, const int32_t* dr, int nd, int dec_dim, ChunkKind kind, int64_t frames) {
    const int bm = 512;
    if (kind == CK_ENCODE) {
        int64_t L = frames;
        for (int i = 0; i < ne; ++i) L *= er[i];
        if (L > ((int64_t)1 << 30)) return false;
        return conv_rows_fit32(bm, pitch16(L), L);   // the longest rows are the stem's; deeper stages only shrink
    }
    if (kind == CK_DECODE) {
        int64_t L = frames;
        for (int i = 0; i < nd; ++i) {
            const int64_t s = dr[i], Lo = L * s, P = pitch16(Lo);
            const int Co = dec_dim >> (i + 1);
            if (!conv_rows_fit32(bm, P, Lo) || !conv_subpixel_fits32(Co, P, (int64_t)Co * P, Lo)) return false;
            L = Lo;
        }
        return true;
    }
    return conv_rows_fit32(bm, frames, frames);   // FromCodes: 1x1 projections at frame rate
}

ChunkPlan make_plan(int64_t setting, const nc_halo& h, ChunkKind kind, int64_t frames, bool fits) {
    ChunkPlan P;
    P.chunk = frames;
    if (setting < 0) return P;                                     // NC_CHUNK_OFF
    int64_t chunk = 0;
    if (setting > 0) chunk = round_up(setting, h.align);
    else if (!fits) chunk = auto_chunk(h, kind == CK_DECODE);      // NC_CHUNK_AUTO: only what one-shot would refuse
    if (chunk <= 0 || frames <= chunk) return P;
    P.chunk = chunk;
    P.n_chunks = ceil_div(frames, chunk);
    if (kind == CK_ENCODE) { P.halo_l = h.enc_right; P.halo_r = h.enc_left; }
    if (kind == CK_DECODE) { P.halo_l = h.dec_right; P.halo_r = h.dec_left; }
    return P;
}

struct Window { int64_t f0, f1, w0, w1; };
Window window_of(const ChunkPlan& P, int64_t j, int64_t frames) {
    Window w;
    w.f0 = j * P.chunk; w.f1 = std::min(frames, w.f0 + P.chunk);
    w.w0 = std::max<int64_t>(0, w.f0 - P.halo_l); w.w1 = std::min(frames, w.f1 + P.halo_r);
    return w;
}
int64_t max_window(const ChunkPlan& P, int64_t frames) { return std::min(frames, P.chunk + P.halo_l + P.halo_r); }

// Plans a call of model m.  True: a device-pointer call that is not cut, which is the *_dev launch sequence on the caller's own arrays
// with no window buffer in between.  Arguments that sequence rejects by itself go there untouched.
template <class M>
bool plan_call(const M& m, bool host, ChunkKind kind, int B, int64_t frames, ChunkPlan& P) {
    if (B > 0 && frames > 0) P = m.chunk_plan(kind, B, frames);
    return !host && P.n_chunks == 1;
}

}  // namespace

void Codec::copy2d(void* dst, bool dst_host, size_t dpitch, const void* src, bool src_host, size_t spitch, size_t width, size_t rows) {
    if (!width || !rows) return;
    if (!dst_host && !src_host) { launch_copy_rows(dst, dpitch, src, spitch, width, rows, stream); return; }
    const hipMemcpyKind kind = dst_host ? (src_host ? hipMemcpyHostToHost : hipMemcpyDeviceToHost) : hipMemcpyHostToDevice;
    if (rows == 1 || (width == dpitch && width == spitch)) NC_HIP(hipMemcpyAsync(dst, src, width * rows, kind, stream));
    else NC_HIP(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, kind, stream));
}

// =============================================================================================== DAC
static void dac_halo(const nc_dac_config& c, nc_halo* out) {
    halo_from_layers(c.encoder_rates, c.n_encoder_rates, c.decoder_rates, c.n_decoder_rates, 1, 0, 1, 1, out);
}

ChunkPlan DacModel::chunk_plan(ChunkKind kind, int B, int64_t Tz) const {
    if (B <= 0 || Tz <= 0) fail(NC_EINVAL, "B and frames must be positive");
    nc_halo h{};
    dac_halo(cfg, &h);
    const bool fits = chunk_frames != 0 || oneshot_fits(cfg.encoder_rates, cfg.n_encoder_rates, cfg.encoder_dim, cfg.decoder_rates,
                                                        cfg.n_decoder_rates, cfg.decoder_dim, kind, Tz);
    ChunkPlan P = make_plan(chunk_frames, h, kind, Tz, fits);
    P.arena_bytes = arena_bytes(cfg, kind, B, P.n_chunks > 1 ? max_window(P, Tz) : Tz);
    return P;
}

// 3 rotating activation buffers of B x max(C * L) floats over the widest window
int64_t DacModel::arena_bytes(const nc_dac_config& cfg, ChunkKind kind, int64_t B, int64_t W) {
    int64_t maxel = 0;
    if (kind == CK_ENCODE) {
        int64_t hop = 1;
        for (int i = 0; i < cfg.n_encoder_rates; ++i) hop *= cfg.encoder_rates[i];
        int c = cfg.encoder_dim;
        int64_t L = W * hop;
        maxel = (int64_t)c * pitch16(L);
        for (int i = 0; i < cfg.n_encoder_rates; ++i) { c *= 2; L /= cfg.encoder_rates[i]; maxel = std::max(maxel, (int64_t)c * pitch16(L)); }
    } else if (kind == CK_DECODE) {
        int64_t L = W;
        maxel = (int64_t)cfg.decoder_dim * pitch16(L);
        for (int i = 0; i < cfg.n_decoder_rates; ++i) { L *= cfg.decoder_rates[i]; maxel = std::max(maxel, (int64_t)(cfg.decoder_dim >> (i + 1)) * pitch16(L)); }
    }
    return 3 * B * maxel * 4;
}

void DacModel::encode(bool host, const float* pcm, int B, int64_t T, int sample_rate, int n_q, int64_t* codes, float* z, float* latents, int64_t* codes_tq) {
    ChunkPlan P;
    if (plan_call(*this, host, CK_ENCODE, B, T > 0 ? frames(T) : 0, P))
        return codes_tq ? encode_code_matrix_dev(pcm, B, T, sample_rate, codes_tq) : encode_dev(pcm, B, T, sample_rate, n_q, codes, z, latents);
    if (!pcm || !(codes || codes_tq)) fail(NC_EINVAL, "pcm and codes must not be null");
    if (B <= 0 || T <= 0) fail(NC_EINVAL, "B and T must be positive");
    if (T > (int64_t)1 << 30) fail(NC_EINVAL, "clip too long");
    use_device();
    const int nq = codes_tq ? cfg.n_codebooks : ((n_q <= 0 || n_q > cfg.n_codebooks) ? cfg.n_codebooks : n_q);
    const int D = cfg.codebook_dim;
    const int64_t Tz = frames(T);
    for (int64_t j = 0; j < P.n_chunks; ++j) {
        const Window w = window_of(P, j, Tz);
        const int64_t s0 = w.w0 * hop, Tw = std::min(T, w.w1 * hop) - s0, Wf = w.w1 - w.w0, k0 = w.f0 - w.w0, n = w.f1 - w.f0;
        ck_in.reserve((size_t)B * Tw * 4);
        ck_codes.reserve((size_t)B * nq * Wf * 8);
        copy2d(ck_in.p, false, (size_t)Tw * 4, pcm + s0, host, (size_t)T * 4, (size_t)Tw * 4, (size_t)B);
        if (codes_tq) {
            encode_code_matrix_dev(ck_in.as<float>(), B, Tw, sample_rate, ck_codes.as<int64_t>());
            copy2d(codes_tq + w.f0 * nq, host, (size_t)Tz * nq * 8, ck_codes.as<int64_t>() + k0 * nq, false, (size_t)Wf * nq * 8, (size_t)n * nq * 8, (size_t)B);
            continue;
        }
        if (z) ck_a.reserve((size_t)B * latent * Wf * 4);
        if (latents) ck_b.reserve((size_t)B * nq * D * Wf * 4);
        encode_dev(ck_in.as<float>(), B, Tw, sample_rate, n_q, ck_codes.as<int64_t>(), z ? ck_a.as<float>() : nullptr, latents ? ck_b.as<float>() : nullptr);
        copy2d(codes + w.f0, host, (size_t)Tz * 8, ck_codes.as<int64_t>() + k0, false, (size_t)Wf * 8, (size_t)n * 8, (size_t)B * nq);
        if (z) copy2d(z + w.f0, host, (size_t)Tz * 4, ck_a.as<float>() + k0, false, (size_t)Wf * 4, (size_t)n * 4, (size_t)B * latent);
        if (latents) copy2d(latents + w.f0, host, (size_t)Tz * 4, ck_b.as<float>() + k0, false, (size_t)Wf * 4, (size_t)n * 4, (size_t)B * nq * D);
    }
}

void DacModel::from_codes(bool host, const int64_t* codes, int B, int n_q, int64_t Tz, float* z) {
    ChunkPlan P;
    if (plan_call(*this, host, CK_FROM_CODES, B, Tz, P)) return from_codes_dev(codes, B, n_q, Tz, z);
    if (!codes || !z) fail(NC_EINVAL, "codes and z must not be null");
    if (B <= 0 || Tz <= 0 || n_q <= 0 || n_q > cfg.n_codebooks) fail(NC_EINVAL, "bad codes shape [%d,%d,%lld]", B, n_q, (long long)Tz);
    use_device();
    for (int64_t j = 0; j < P.n_chunks; ++j) {   // per frame: no halo
        const Window w = window_of(P, j, Tz);
        const int64_t n = w.f1 - w.f0;
        ck_codes.reserve((size_t)B * n_q * n * 8);
        ck_a.reserve((size_t)B * latent * n * 4);
        copy2d(ck_codes.p, false, (size_t)n * 8, codes + w.f0, host, (size_t)Tz * 8, (size_t)n * 8, (size_t)B * n_q);
        from_codes_dev(ck_codes.as<int64_t>(), B, n_q, n, ck_a.as<float>());
        copy2d(z + w.f0, host, (size_t)Tz * 4, ck_a.p, false, (size_t)n * 4, (size_t)n * 4, (size_t)B * latent);
    }
}

void DacModel::decode(bool host, const float* z, const int64_t* codes_tq, int n_q, int B, int64_t Tz, float* pcm) {
    ChunkPlan P;
    if (plan_call(*this, host, CK_DECODE, B, Tz, P)) return codes_tq ? decode_code_matrix_dev(codes_tq, B, Tz, n_q, pcm) : decode_dev(z, B, Tz, pcm);
    if (!(z || codes_tq) || !pcm) fail(NC_EINVAL, "z and pcm must not be null");
    if (B <= 0 || Tz <= 0) fail(NC_EINVAL, "B and frames must be positive");
    if (codes_tq && (n_q <= 0 || n_q > cfg.n_codebooks)) fail(NC_EINVAL, "bad code matrix shape [%d,%lld,%d]", B, (long long)Tz, n_q);
    use_device();
    int64_t H = 1;   // output samples per frame: every block maps L -> L*s - (s odd), so a window's samples sit at frame * H exactly
    for (int i = 0; i < cfg.n_decoder_rates; ++i) H *= cfg.decoder_rates[i];
    const int64_t Lfull = decoded_len(Tz);
    for (int64_t j = 0; j < P.n_chunks; ++j) {
        const Window w = window_of(P, j, Tz);
        const int64_t Wf = w.w1 - w.w0, Lw = decoded_len(Wf), o0 = w.f0 * H, o1 = w.f1 == Tz ? Lfull : w.f1 * H, k0 = (w.f0 - w.w0) * H;
        if (o1 <= o0) continue;
        if (k0 + (o1 - o0) > Lw) fail(NC_ESTATE, "internal: decoded window of %lld samples does not cover its chunk", (long long)Lw);
        ck_out.reserve((size_t)B * Lw * 4);
        if (codes_tq) {
            ck_codes.reserve((size_t)B * Wf * n_q * 8);
            copy2d(ck_codes.p, false, (size_t)Wf * n_q * 8, codes_tq + w.w0 * n_q, host, (size_t)Tz * n_q * 8, (size_t)Wf * n_q * 8, (size_t)B);
            decode_code_matrix_dev(ck_codes.as<int64_t>(), B, Wf, n_q, ck_out.as<float>());
        } else {
            ck_a.reserve((size_t)B * latent * Wf * 4);
            copy2d(ck_a.p, false, (size_t)Wf * 4, z + w.w0, host, (size_t)Tz * 4, (size_t)Wf * 4, (size_t)B * latent);
            decode_dev(ck_a.as<float>(), B, Wf, ck_out.as<float>());
        }
        copy2d(pcm + o0, host, (size_t)Lfull * 4, ck_out.as<float>() + k0, false, (size_t)Lw * 4, (size_t)(o1 - o0) * 4, (size_t)B);
    }
}

// ============================================================================================== SNAC
static void snac_halo(const nc_snac_config& c, nc_halo* out) {
    if (c.n_vq_strides <= 0 || c.n_vq_strides > 8) fail(NC_EINVAL, "vq stride list must hold 1..8 entries");
    const int W = c.attn_window_size > 0 ? c.attn_window_size : 1;
    int64_t a = c.vq_strides[0], x = a, y = W;
    if (a <= 0) fail(NC_EINVAL, "vq stride must be positive");
    while (y) { const int64_t t = x % y; x = y; y = t; }
    const int64_t align = a / x * W;
    int vq_max = 1;
    for (int i = 0; i < c.n_vq_strides; ++i) {
        if (c.vq_strides[i] <= 0) fail(NC_EINVAL, "vq stride must be positive");
        if (align % c.vq_strides[i] != 0) fail(NC_EUNSUPPORTED, "vq stride %d does not divide lcm(vq_strides[0], attention window) = %lld", c.vq_strides[i], (long long)align);
        vq_max = std::max(vq_max, (int)c.vq_strides[i]);
    }
    halo_from_layers(c.encoder_rates, c.n_encoder_rates, c.decoder_rates, c.n_decoder_rates, 3, W, vq_max, align, out);
}

ChunkPlan SnacModel::chunk_plan(ChunkKind kind, int B, int64_t frames_in) const {
    if (B <= 0 || frames_in <= 0) fail(NC_EINVAL, "B and frames must be positive");
    nc_halo h{};
    snac_halo(cfg, &h);
    const int64_t Tz = round_up(frames_in, h.align);
    const bool fits = chunk_frames != 0 || oneshot_fits(cfg.encoder_rates, cfg.n_encoder_rates, cfg.encoder_dim, cfg.decoder_rates,
                                                        cfg.n_decoder_rates, cfg.decoder_dim, kind, Tz);
    ChunkPlan P = make_plan(chunk_frames, h, kind, Tz, fits);
    P.arena_bytes = arena_bytes(cfg, kind, B, P.n_chunks > 1 ? max_window(P, Tz) : Tz);
    return P;
}

int64_t SnacModel::arena_bytes(const nc_snac_config& cfg, ChunkKind kind, int64_t B, int64_t W) {
    int64_t maxel = 0;   // reserve_act: the widest tensor of either direction
    if (kind != CK_FROM_CODES) {
        int64_t hop = 1;
        for (int i = 0; i < cfg.n_encoder_rates; ++i) hop *= cfg.encoder_rates[i];
        int c = cfg.encoder_dim;
        int64_t L = W * hop;
        maxel = (int64_t)c * L;
        for (int i = 0; i < cfg.n_encoder_rates; ++i) { c *= 2; L /= cfg.encoder_rates[i]; maxel = std::max(maxel, (int64_t)c * L); }
        int64_t Ld = W;
        maxel = std::max(maxel, (int64_t)cfg.decoder_dim * Ld);
        for (int i = 0; i < cfg.n_decoder_rates; ++i) { Ld = up_len(Ld, cfg.decoder_rates[i]); maxel = std::max(maxel, (int64_t)(cfg.decoder_dim >> (i + 1)) * Ld); }
    }
    return 3 * B * maxel * 4;
}

void SnacModel::copy_levels(int64_t* dst, bool dst_host, int64_t Td, int64_t d0, const int64_t* src, bool src_host, int64_t Ts, int64_t s0, int64_t n, int B) {
    const int64_t td = codes_per_clip(Td), ts = codes_per_clip(Ts);
    if (n == Td && n == Ts) return copy2d(dst, dst_host, (size_t)td * 8, src, src_host, (size_t)ts * 8, (size_t)td * 8, (size_t)B);   // the window is the clip: the level blocks coincide
    int64_t od = 0, os = 0;
    for (int i = 0; i < cfg.n_vq_strides; ++i) {   // every level at its own rate
        const int s = cfg.vq_strides[i];
        copy2d(dst + od + d0 / s, dst_host, (size_t)td * 8, src + os + s0 / s, src_host, (size_t)ts * 8, (size_t)(n / s) * 8, (size_t)B);
        od += Td / s; os += Ts / s;
    }
}

void SnacModel::encode(bool host, const float* pcm, int B, int64_t T, int64_t* codes, float* z, float* zq) {
    ChunkPlan P;
    if (plan_call(*this, host, CK_ENCODE, B, T > 0 ? padded_len(T) / hop : 0, P)) return encode_dev(pcm, B, T, codes, z, zq);
    if (!pcm || !codes) fail(NC_EINVAL, "pcm and codes must not be null");
    if (B <= 0 || T <= 0 || T > ((int64_t)1 << 30)) fail(NC_EINVAL, "B and T must be positive");
    use_device();
    const int64_t Tz = padded_len(T) / hop;
    for (int64_t j = 0; j < P.n_chunks; ++j) {
        const Window w = window_of(P, j, Tz);
        const int64_t s0 = w.w0 * hop, Tw = std::min(T, w.w1 * hop) - s0, Wf = w.w1 - w.w0, k0 = w.f0 - w.w0, n = w.f1 - w.f0;
        if (Tw <= 0 || padded_len(Tw) / hop != Wf) fail(NC_ESTATE, "internal: window of %lld samples does not give %lld frames", (long long)Tw, (long long)Wf);
        ck_in.reserve((size_t)B * Tw * 4);
        ck_codes.reserve((size_t)B * codes_per_clip(Wf) * 8);
        if (z) ck_a.reserve((size_t)B * latent * Wf * 4);
        if (zq) ck_b.reserve((size_t)B * latent * Wf * 4);
        copy2d(ck_in.p, false, (size_t)Tw * 4, pcm + s0, host, (size_t)T * 4, (size_t)Tw * 4, (size_t)B);
        encode_dev(ck_in.as<float>(), B, Tw, ck_codes.as<int64_t>(), z ? ck_a.as<float>() : nullptr, zq ? ck_b.as<float>() : nullptr, true);
        copy_levels(codes, host, Tz, w.f0, ck_codes.as<int64_t>(), false, Wf, k0, n, B);
        if (z) copy2d(z + w.f0, host, (size_t)Tz * 4, ck_a.as<float>() + k0, false, (size_t)Wf * 4, (size_t)n * 4, (size_t)B * latent);
        if (zq) copy2d(zq + w.f0, host, (size_t)Tz * 4, ck_b.as<float>() + k0, false, (size_t)Wf * 4, (size_t)n * 4, (size_t)B * latent);
    }
}

void SnacModel::from_codes(bool host, const int64_t* codes, int B, int64_t Tz, float* zq_out) {
    ChunkPlan P;
    if (plan_call(*this, host, CK_FROM_CODES, B, Tz, P)) return from_codes_dev(codes, B, Tz, zq_out);
    if (!codes || !zq_out) fail(NC_EINVAL, "codes and zq must not be null");
    if (B <= 0 || Tz <= 0) fail(NC_EINVAL, "B and frames must be positive");
    for (int i = 0; i < cfg.n_vq_strides; ++i)
        if (Tz % cfg.vq_strides[i] != 0) fail(NC_EINVAL, "frame count %lld is not a multiple of vq stride %d", (long long)Tz, cfg.vq_strides[i]);
    use_device();
    for (int64_t j = 0; j < P.n_chunks; ++j) {   // per pooling block: no halo, boundaries are multiples of align
        const Window w = window_of(P, j, Tz);
        const int64_t n = w.f1 - w.f0;
        ck_codes.reserve((size_t)B * codes_per_clip(n) * 8);
        ck_a.reserve((size_t)B * latent * n * 4);
        copy_levels(ck_codes.as<int64_t>(), false, n, 0, codes, host, Tz, w.f0, n, B);
        from_codes_dev(ck_codes.as<int64_t>(), B, n, ck_a.as<float>());
        copy2d(zq_out + w.f0, host, (size_t)Tz * 4, ck_a.p, false, (size_t)n * 4, (size_t)n * 4, (size_t)B * latent);
    }
}

void SnacModel::decode(bool host, const int64_t* codes, int B, int64_t Tz, const float* noise, uint64_t seed, float* pcm) {
    ChunkPlan P;
    if (plan_call(*this, host, CK_DECODE, B, Tz, P)) return decode_dev(codes, B, Tz, noise, seed, pcm);
    if (!codes || !pcm) fail(NC_EINVAL, "codes and pcm must not be null");
    if (B <= 0 || Tz <= 0) fail(NC_EINVAL, "B and frames must be positive");
    for (int i = 0; i < cfg.n_vq_strides; ++i)
        if (Tz % cfg.vq_strides[i] != 0) fail(NC_EINVAL, "frame count %lld is not a multiple of vq stride %d", (long long)Tz, cfg.vq_strides[i]);
    use_device();
    // NoiseBlock inputs: one [B,1,T_i] block per decoder stage, T_i = frames * (product of the strides so far).  A window takes its
    // slice of the caller's noise.  Without caller noise a window that is the whole clip leaves the draw from `seed` to the launch
    // sequence; any other window slices the whole clip's noise, drawn once exactly as the launch sequence draws it (about the size of
    // the PCM).
    const float* nz = noise;
    bool nz_host = host;
    const int64_t Lfull = decoded_len(Tz);   // = Tz * hop: every SNAC up-conv maps L -> L * s
    for (int64_t j = 0; j < P.n_chunks; ++j) {
        const Window w = window_of(P, j, Tz);
        const int64_t Wf = w.w1 - w.w0, Lw = decoded_len(Wf);
        ck_codes.reserve((size_t)B * codes_per_clip(Wf) * 8);
        copy_levels(ck_codes.as<int64_t>(), false, Wf, 0, codes, host, Tz, w.w0, Wf, B);
        const bool slice = cfg.noise && (noise || Wf != Tz);
        if (slice) {
            if (!nz) {
                const int64_t n = noise_len(B, Tz);
                ck_noise_full.reserve((size_t)n * 4);
                launch_randn(ck_noise_full.as<float>(), n, seed, stream);
                nz = ck_noise_full.as<float>();
                nz_host = false;
            }
            const size_t n_w = (size_t)noise_len(B, Wf) * 4;
            ck_noise.reserve(n_w);
            if (Wf == Tz) {   // the window is the clip: the stage blocks coincide
                copy2d(ck_noise.p, false, n_w, nz, nz_host, n_w, n_w, 1);
            } else {
                int64_t S = 1, off = 0, off_w = 0;
                for (int i = 0; i < cfg.n_decoder_rates; ++i) {
                    S *= cfg.decoder_rates[i];
                    copy2d(ck_noise.as<float>() + off_w, false, (size_t)Wf * S * 4, nz + off + w.w0 * S, nz_host, (size_t)Tz * S * 4, (size_t)Wf * S * 4, (size_t)B);
                    off += (int64_t)B * Tz * S; off_w += (int64_t)B * Wf * S;
                }
            }
        }
        ck_out.reserve((size_t)B * Lw * 4);
        decode_dev(ck_codes.as<int64_t>(), B, Wf, slice ? ck_noise.as<float>() : nullptr, seed, ck_out.as<float>());
        const int64_t Hs = Lfull / Tz, o0 = w.f0 * Hs, cnt = (w.f1 - w.f0) * Hs, k0 = (w.f0 - w.w0) * Hs;
        copy2d(pcm + o0, host, (size_t)Lfull * 4, ck_out.as<float>() + k0, false, (size_t)Lw * 4, (size_t)cnt * 4, (size_t)B);
    }
}

}  // namespace nc

// ================================================================================================ C ABI
using namespace nc;

extern "C" {

nc_status nc_dac_halo(const nc_dac_config* cfg, nc_halo* out) {
    return guard([&] {
        if (!cfg || !out) fail(NC_EINVAL, "cfg and out must not be null");
        dac_halo(*cfg, out);
    });
}

nc_status nc_snac_halo(const nc_snac_config* cfg, nc_halo* out) {
    return guard([&] {
        if (!cfg || !out) fail(NC_EINVAL, "cfg and out must not be null");
        if (cfg->attn_window_size < 0 || cfg->attn_window_size > 32) fail(NC_EINVAL, "attention window must be in 0..32");
        snac_halo(*cfg, out);
    });
}

nc_status nc_codec_set_chunk_frames(nc_codec* h, int64_t chunk_frames) {
    return guard([&] {
        Codec& c = codec_of(h);
        if (h->kind == EncodecModel::kKind) fail(NC_EUNSUPPORTED, "Encodec handles are not chunked: 48 kHz is segmented per second already, the 24 kHz LSTM has unbounded context");
        if (chunk_frames < NC_CHUNK_OFF) fail(NC_EINVAL, "chunk_frames must be NC_CHUNK_OFF (-1), NC_CHUNK_AUTO (0) or a positive frame count");
        c.chunk_frames = chunk_frames;
    });
}

nc_status nc_codec_chunk_plan(const nc_codec* h, int32_t decode, int32_t B, int64_t frames, nc_chunk_plan* out) {
    return guard([&] {
        if (!h || !h->impl || !out) fail(NC_EINVAL, "null argument");
        if (h->kind == EncodecModel::kKind) fail(NC_EUNSUPPORTED, "Encodec handles are not chunked");
        if (B <= 0 || frames <= 0) fail(NC_EINVAL, "B and frames must be positive");
        const ChunkKind kind = decode ? CK_DECODE : CK_ENCODE;
        const ChunkPlan P = h->kind == DacModel::kKind ? as<DacModel>(h).chunk_plan(kind, B, frames) : as<SnacModel>(h).chunk_plan(kind, B, frames);
        out->n_chunks = P.n_chunks; out->chunk_frames = P.chunk; out->halo_left = P.halo_l; out->halo_right = P.halo_r;
        out->arena_bytes = P.arena_bytes;
    });
}

}  // extern "C"
