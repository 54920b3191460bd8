/* nc_mi355x.h -- C ABI of the MI355X-native neural-audio-codec engine (libnc_mi355x.so).
 *
 * This is the drop-in boundary for the reference's Encode/Decode hot path.  The reference
 * (DillionLowry/NeuralCodecs, C#/.NET 8 on TorchSharp) has no FFI of its own for this path:
 * every op is a TorchSharp P/Invoke into libtorch.  The functions below are what a C# shim
 * binds with [DllImport("nc_mi355x")] to keep the managed API surface
 * (INeuralCodec, DAC.Encode/Decode/FromCodes, SNAC.Encode/Decode, Encodec.Encode/Decode)
 * while every FLOP runs in hand-written HIP kernels for gfx950.  See INTEGRATION.md.
 *
 * Conventions
 *   - plain C types only; tensors are dense row-major float32 [B,C,T] / int64 codes [B,Nq,T'].
 *   - every function returns nc_status; nc_last_error() gives the thread-local message.
 *     Mapping to the reference's exceptions: NC_EINVAL -> ArgumentException /
 *     ArgumentNullException, NC_ENOTFOUND -> FileNotFoundException, NC_ESTATE ->
 *     InvalidOperationException, NC_EDEVICE / NC_ENOMEM -> NeuralCodecException.
 *   - one handle = one device + one HIP stream; calls on one handle must be serialised by the
 *     caller (the reference's modules are not thread-safe either: WNConv1d.cs:150 mutates state
 *     in forward); distinct handles may run concurrently.
 *   - "*_dev" variants take DEVICE pointers, enqueue on the handle's stream and return without
 *     synchronising (zero-copy path used by benchmarks / multi-GPU sharding); the plain variants
 *     take HOST pointers and are synchronous (the float[] / Tensor overloads of the reference).
 *   - there is NO CPU fallback: every entry point fails with NC_EDEVICE when no gfx950 device
 *     is usable.
 */
#ifndef NC_MI355X_H
#define NC_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NC_API __attribute__((visibility("default")))

typedef enum {
    NC_OK = 0,
    NC_EINVAL = 1,     /* bad argument (null pointer, wrong sample rate, bad shape) */
    NC_ENOTFOUND = 2,  /* weight file / tensor not found */
    NC_ESTATE = 3,     /* call not valid in this state (weights not loaded, ...) */
    NC_EDEVICE = 4,    /* HIP error / no usable device */
    NC_ENOMEM = 5,
    NC_EUNSUPPORTED = 6
} nc_status;

typedef struct nc_codec nc_codec; /* opaque: replaces the managed DAC / SNAC / Encodec object (INeuralCodec + IDisposable,
                                     NeuralCodecs.Core/INeuralCodec.cs:8-20) */

NC_API const char* nc_last_error(void);
NC_API const char* nc_version(void);
/* number of HIP devices visible (0 when none); never fails */
NC_API int nc_device_count(void);
/* Every diagnostic environment switch the engine reads, one "NAME\tkind\twhat it does\n" line each; kind b = set to 1,
 * p = set at all, i = integer, s = string.  None of them changes a result (every path is bit-exact against the oracle); they exist so
 * that an A/B on one box is one environment variable.  The engine refuses to read a switch that is not in this table. */
NC_API const char* nc_debug_switches(void);

/* ------------------------------------------------------------------------------------------ DAC
 * replaces: new DAC(DACConfig)                    NeuralCodecs.Torch/Models/DAC.cs:51-93
 *           fields consumed                       NeuralCodecs.Torch/Config/DAC/DACConfig.cs:22-76 */
typedef struct {
    int32_t sample_rate;     /* 44100 */
    int32_t encoder_dim;     /* 64 */
    int32_t n_encoder_rates; /* 4 */
    int32_t encoder_rates[8];/* 2,4,8,8 */
    int32_t decoder_dim;     /* 1536 */
    int32_t n_decoder_rates; /* 4 */
    int32_t decoder_rates[8];/* 8,8,4,2 */
    int32_t latent_dim;      /* 0 => encoder_dim * 2^n_encoder_rates (DAC.cs:64) */
    int32_t n_codebooks;     /* 9 */
    int32_t codebook_size;   /* 1024 */
    int32_t codebook_dim;    /* 8 */
} nc_dac_config;

NC_API nc_status nc_dac_create(const nc_dac_config* cfg, int device_index, nc_codec** out);

/* replaces: IDisposable.Dispose                   Models/DAC.cs:329-338 */
NC_API nc_status nc_codec_destroy(nc_codec* h);

/* replaces: INeuralCodec.LoadWeights(path)        Models/DAC.cs:345-389 (FileNotFound / InvalidOperation)
 * The file is an NCWB0001 weight blob whose tensor names are the reference's TorchSharp
 * state-dict keys (weight_v / weight_g / bias / alpha / codebook.weight); the
 * weight-norm fold w = v/(||v||+1e-7)*g (WNConv1d.cs:145-150) happens once here. */
NC_API nc_status nc_codec_load_weights(nc_codec* h, const char* path);
NC_API nc_status nc_codec_load_weights_mem(nc_codec* h, const void* blob, size_t nbytes);
/* Host-only validation of an NCWB0001 image (what the two loaders run first): every index field bounds-checked, (offset, size) pairs
 * checked without overflow, dtype / byte-count consistency.  NC_EINVAL on a truncated or crafted image; needs no device. */
NC_API nc_status nc_blob_check(const void* blob, size_t nbytes, int32_t* n_tensors);

/* Run the handle's work on a caller-owned hipStream_t.  NULL is HIP's legacy default (null) stream -- the stream PyTorch-ROCm
 * uses by default -- so device buffers produced by the caller's framework are ordered with the engine's kernels.
 * nc_codec_reset_stream returns to the handle's own (non-blocking) stream. */
NC_API nc_status nc_codec_set_stream(nc_codec* h, void* hip_stream);
NC_API nc_status nc_codec_reset_stream(nc_codec* h);
NC_API nc_status nc_codec_synchronize(nc_codec* h);
/* Errors raised by device code after a device-pointer call returned (today: the bounded spins of Encodec's persistent LSTM kernel, which
 * needs its workgroups co-resident).  Non-blocking: call it once the caller knows the stream is idle (after its own stream / device
 * synchronisation); nc_codec_synchronize and the host-pointer entry points check by themselves, and every device-pointer call checks
 * for a failure of the previous one first.  NC_EDEVICE = the results of that call are invalid; the handle has switched to the
 * step-wise kernels, so repeating the call succeeds (the host-pointer entry points repeat it themselves). */
NC_API nc_status nc_codec_check_errors(nc_codec* h);
/* Encodec handles: which LSTM kernels the handle runs (SLSTM.cs:40-57) -- *stepwise = 1 once a persistent launch has timed out (or the
 * device cannot hold one) -- and how many such timeouts this handle has seen.  Persistent LSTM sections of DIFFERENT handles on one
 * device are ordered one after the other on the GPU (a per-device ticket inside the engine: their workgroups must be co-resident and two
 * handles' worth do not fit), so concurrent handles keep the persistent kernels; only other PROCESSES sharing the device can starve them. */
NC_API nc_status nc_encodec_lstm_stats(const nc_codec* h, int32_t* stepwise, int64_t* timeouts);

/* Shape helper for DAC.Preprocess (Models/DAC.cs:141-154): padded length and frame count T'. */
NC_API nc_status nc_dac_query(const nc_codec* h, int64_t T, int64_t* T_padded, int64_t* frames);

/* replaces: DAC.Encode(Tensor audio[B,1,T], int? nQuantizers, int? sampleRate)   Models/DAC.cs:163-181
 *   pcm        [B,1,T] float32
 *   sample_rate 0 = model rate; a mismatch returns NC_EINVAL (ArgumentException, DAC.cs:146)
 *   n_q        0 = all codebooks (the null overload, ResidualVectorQuantizer.cs:54-103)
 *   codes      [B,n_q,T'] int64            (required)
 *   z          [B,latent,T'] float32       (nullable; the quantized latents zQ)
 *   latents    [B,n_q*codebook_dim,T']     (nullable; the projected latents zE)
 * The two loss outputs of the reference are constant 0 in inference (D5) and are not returned. */
NC_API nc_status nc_dac_encode(nc_codec* h, const float* pcm, int32_t B, int64_t T, int32_t sample_rate, int32_t n_q,
                               int64_t* codes, float* z, float* latents);
NC_API nc_status nc_dac_encode_dev(nc_codec* h, const float* pcm, int32_t B, int64_t T, int32_t sample_rate, int32_t n_q,
                                   int64_t* codes, float* z, float* latents);

/* replaces: DAC.Decode(Tensor z[B,latent,T'])  -> [B,1,L]   Models/DAC.cs:231-234 (no trim: D6).  L = T'*hop when every decoder stride is
 * even (the 44.1 kHz presets); each DecoderBlock maps L -> (L - 1) s - 2 ceil(s / 2) + 2 s (DecoderBlock.cs:20-44), so a stride-5 block
 * (the 16 / 24 kHz presets, DACConfig.cs:115-135) yields 5 L - 1: a caller sizes `pcm` for T'*hop (= nc_dac_query's T_padded), never less. */
NC_API nc_status nc_dac_decode(nc_codec* h, const float* z, int32_t B, int64_t frames, float* pcm);
NC_API nc_status nc_dac_decode_dev(nc_codec* h, const float* z, int32_t B, int64_t frames, float* pcm);

/* replaces: DAC.FromCodes(Tensor codes[B,n_q,T']) -> z[B,latent,T']   Models/DAC.cs:101-106 */
NC_API nc_status nc_dac_from_codes(nc_codec* h, const int64_t* codes, int32_t B, int32_t n_q, int64_t frames, float* z);
NC_API nc_status nc_dac_from_codes_dev(nc_codec* h, const int64_t* codes, int32_t B, int32_t n_q, int64_t frames, float* z);

/* replaces: ResidualVectorQuantizer.FromLatents(Tensor latents[B,C_lat,T']) -> (zQ, projected, codes)
 *           Modules/DAC/ResidualVectorQuantizer.cs:243-300 over VectorQuantizer.DecodeLatents (VectorQuantizer.cs:99-125)
 * The way back in for the continuous `latents` that nc_dac_encode hands out: every codebook slice of D = codebook_dim channels is
 * looked up in its codebook (nearest code on the un-normalised vectors; lowest index on ties, a NaN distance wins, the first one --
 * the rules of the encoder's quantizer, so latents taken from nc_dac_encode return its codes unchanged), the raw codebook rows are
 * out-projected and summed as nc_dac_from_codes sums them (z is bit-identical to nc_dac_from_codes on the returned codes).
 *   latents    [B,C_lat,T'] float32; n_q = min(n_codebooks, C_lat / D) codebooks are used (those whose cumulative dimension fits);
 *              channels beyond n_q*D are ignored, the row stride stays C_lat
 *   z          [B,latent,T'] float32       (nullable)
 *   projected  [B,n_q*D,T'] float32        (nullable; the raw codebook rows, the reference's cat(projected))
 *   codes      [B,n_q,T'] int64            (nullable)
 * NC_EINVAL, before anything is launched: latents NULL; all three outputs NULL; B <= 0; frames <= 0; frames > 2^30; C_lat < D (the
 * reference would return a one-element zero tensor there, which no caller can use: a deliberate deviation).  NC_ESTATE without weights.
 * The operation is pointwise in time (no halo) and addresses batch and frame offsets in 64 bits, so no size is refused; the
 * out-projection of rows too long for one convolution launch is cut as nc_dac_from_codes cuts it (nc_codec_set_chunk_frames applies).
 * Clips of unequal lengths need no entry point of their own: packed end to end along T' they are one B = 1 call. */
NC_API nc_status nc_dac_from_latents(nc_codec* h, const float* latents, int32_t B, int32_t C_lat, int64_t frames, float* z,
                                     float* projected, int64_t* codes);
NC_API nc_status nc_dac_from_latents_dev(nc_codec* h, const float* latents, int32_t B, int32_t C_lat, int64_t frames, float* z,
                                         float* projected, int64_t* codes);

/* replaces: Dia.Decode(Tensor audioCodes[T, n_q])  Models/Dia.cs:973-981 (FromCodes(codes.unsqueeze(0).transpose(1, 2)) -> Decode) and
 *           AudioUtils.Decode(DAC, codes)           Modules/Dia/AudioUtils.cs:189-199, batched: codes_tq int64 [B, T', n_q] (Dia's layout)
 *           -> pcm [B, 1, L] (L as for nc_dac_decode).  The transpose to DAC's [B, n_q, T'] is a device kernel.
 * replaces: Dia.Encode(Tensor audio[1, T])          Models/Dia.cs:989-1002 (Encode -> squeeze(0).transpose(0, 1)), batched:
 *           pcm [B, 1, T] -> codes_tq int64 [B, T', n_q] (all codebooks) */
NC_API nc_status nc_dac_decode_code_matrix(nc_codec* h, const int64_t* codes_tq, int32_t B, int64_t frames, int32_t n_q, float* pcm);
NC_API nc_status nc_dac_decode_code_matrix_dev(nc_codec* h, const int64_t* codes_tq, int32_t B, int64_t frames, int32_t n_q, float* pcm);
NC_API nc_status nc_dac_encode_code_matrix(nc_codec* h, const float* pcm, int32_t B, int64_t T, int32_t sample_rate, int64_t* codes_tq);
NC_API nc_status nc_dac_encode_code_matrix_dev(nc_codec* h, const float* pcm, int32_t B, int64_t T, int32_t sample_rate, int64_t* codes_tq);

/* ----------------------------------------------------------------------------------------- SNAC
 * replaces: new SNAC(SNACConfig)                   NeuralCodecs.Torch/Models/SNAC.cs:34-63
 *           fields consumed                        NeuralCodecs.Torch/Config/SNAC/SNACConfig.cs:40-100 */
typedef struct {
    int32_t sample_rate;      /* 24000 */
    int32_t encoder_dim;      /* 48 */
    int32_t n_encoder_rates;  /* 4 */
    int32_t encoder_rates[8]; /* 2,4,8,8 */
    int32_t decoder_dim;      /* 1024 */
    int32_t n_decoder_rates;
    int32_t decoder_rates[8]; /* 8,8,4,2 */
    int32_t latent_dim;       /* 0 => encoder_dim * 2^n_encoder_rates (SNAC.cs:41) */
    int32_t attn_window_size; /* 0 = no LocalMHA (24 kHz); 32 for the 32/44 kHz presets */
    int32_t codebook_size;    /* 4096 */
    int32_t codebook_dim;     /* 8 */
    int32_t n_vq_strides;
    int32_t vq_strides[8];    /* 4,2,1 */
    int32_t noise;            /* NoiseBlock in every decoder block */
    int32_t depthwise;        /* depthwise k7 convolutions */
} nc_snac_config;

NC_API nc_status nc_snac_create(const nc_snac_config* cfg, int device_index, nc_codec** out);

/* Shape helper for SNAC.Preprocess (Models/SNAC.cs:70-80): padded length = multiple of hop*lcm(vq_strides[0], window),
 * frames T' = padded/hop, per-level code widths T'/stride_i (level_widths has room for 8), decoded length. */
NC_API nc_status nc_snac_query(const nc_codec* h, int64_t T, int64_t* T_padded, int64_t* frames, int32_t* n_levels,
                               int64_t* level_widths, int64_t* decoded_len);

/* replaces: SNAC.Encode(float[])   Models/SNAC.cs:129-150 and the encode half of forward :91-106  (Preprocess pads; for the
 * Tensor overload exactly as written see nc_snac_encode_tensor below; the two agree on lengths that are already multiples)
 *   pcm   [B,1,T] float32
 *   codes [B, sum_i T'/stride_i] int64: the levels of one clip side by side, coarse first (the reference returns a List of
 *         [B, T'/stride_i] tensors; nc_snac_query gives the widths)
 *   z / zq nullable [B, latent, T']: encoder output / quantized latents */
NC_API nc_status nc_snac_encode(nc_codec* h, const float* pcm, int32_t B, int64_t T, int64_t* codes, float* z, float* zq);
NC_API nc_status nc_snac_encode_dev(nc_codec* h, const float* pcm, int32_t B, int64_t T, int64_t* codes, float* z, float* zq);

/* replaces: SNAC.Encode(Tensor) AS WRITTEN   Models/SNAC.cs:113-122 (deviation D7: Preprocess's result is dropped and the encoder
 * runs on the UN-padded tensor).  Frames T' follow the strided convs' floor lengths (nc_snac_query_tensor); where the reference
 * throws (T' not a multiple of every vq stride: repeat_interleave + add shape mismatch, VectorQuantizer.cs:99-101; LocalMHA
 * window reshape, LocalMHA.cs:84-91) the call returns NC_EINVAL.  Same buffer layout as nc_snac_encode with T' from the query. */
NC_API nc_status nc_snac_query_tensor(const nc_codec* h, int64_t T, int64_t* frames, int32_t* n_levels, int64_t* level_widths);
NC_API nc_status nc_snac_encode_tensor(nc_codec* h, const float* pcm, int32_t B, int64_t T, int64_t* codes, float* z, float* zq);
NC_API nc_status nc_snac_encode_tensor_dev(nc_codec* h, const float* pcm, int32_t B, int64_t T, int64_t* codes, float* z, float* zq);

/* replaces: ResidualVectorQuantizer.FromCodes      Modules/SNAC/ResidualVectorQuantizer.cs:100-135 */
NC_API nc_status nc_snac_from_codes(nc_codec* h, const int64_t* codes, int32_t B, int64_t frames, float* zq);
NC_API nc_status nc_snac_from_codes_dev(nc_codec* h, const int64_t* codes, int32_t B, int64_t frames, float* zq);

/* replaces: SNAC.Decode(List<Tensor> codes)        Models/SNAC.cs:157-192 -> [B,1,decoded_len]
 *   noise: the NoiseBlock inputs, one [B,1,T_i] block per decoder stage laid end to end (reference: torch.randn at inference,
 *          NoiseBlock.cs:41, hence not reproducible); NULL = draw N(0,1) on the device from `seed` (counter-based). */
NC_API nc_status nc_snac_decode(nc_codec* h, const int64_t* codes, int32_t B, int64_t frames, const float* noise, uint64_t seed,
                                float* pcm);
NC_API nc_status nc_snac_decode_dev(nc_codec* h, const int64_t* codes, int32_t B, int64_t frames, const float* noise,
                                    uint64_t seed, float* pcm);
/* total number of noise floats nc_snac_decode consumes for (B, frames) */
NC_API nc_status nc_snac_noise_len(const nc_codec* h, int32_t B, int64_t frames, int64_t* n);

/* replaces: SNAC.ProcessAudio(float[] audioData, int sampleRate)   Models/SNAC.cs:255-282 with ResampleAudio :284-308
 * One upload, then resample (when sample_rate differs from the model's; binary64 position arithmetic as nc_audio_resample_linear_dev)
 * -> forward (Preprocess pad, encode, quantize, decode, narrow to the resampled length: SNAC.cs:91-106) on the device, one download.
 *   audio [n] float32 mono; NULL or n <= 0 -> NC_EINVAL (ArgumentException "Audio data cannot be empty", SNAC.cs:257-258)
 *   noise / seed as nc_snac_decode (frames from nc_snac_query on the resampled length, B = 1)
 *   out   [n_out], n_out from nc_snac_process_audio_len (= n when the rates agree, else nc_audio_resample_len) */
NC_API nc_status nc_snac_process_audio_len(const nc_codec* h, int64_t n, int32_t sample_rate, int64_t* n_out);
NC_API nc_status nc_snac_process_audio(nc_codec* h, const float* audio, int64_t n, int32_t sample_rate, const float* noise, uint64_t seed,
                                       float* out);

/* ------------------------------------------------------------------------------------ long clips
 * One-shot size limit.  The convolution kernels address a layer's output with 32-bit offsets, so a one-shot call is refused with
 * NC_EUNSUPPORTED once a layer has (rows of a tile + 4) * row_length + row_length >= 2^31, or, for the up-convolutions,
 * (4 * Cout + 5) * row_length >= 2^31: about two minutes of DAC-44.1k / SNAC-44k audio per clip, whatever B.  Below that limit the
 * activation arena of a one-shot call still grows with the clip (3 * B * max(C * L) * 4 bytes: about 3.4 GB per minute of DAC-44.1k
 * decode at B = 1).
 * DAC and SNAC have a finite receptive field, so a clip can be run in chunks of latent frames with a halo of recomputed frames on
 * each side; every kept output is the number the one-shot call produces, bit for bit.  nc_dac_halo / nc_snac_halo derive the halo in
 * closed form from the config alone (host functions: no handle, no device):
 *   enc_left / enc_right   how many frames before / after its own frame a change of one input sample can move the encoder output
 *   dec_left / dec_right   the same for a change of one latent frame and the output samples, in frames of hop samples
 *   align                  chunk boundaries are multiples of this (SNAC: lcm(vq_strides[0], attention window); DAC: 1)
 * Every halo is a multiple of align.  A chunk needs to its LEFT what a change reaches to its RIGHT, and the other way round. */
typedef struct nc_halo {
    int64_t enc_left, enc_right;
    int64_t dec_left, dec_right;
    int64_t align;
} nc_halo;
NC_API nc_status nc_dac_halo(const nc_dac_config* cfg, nc_halo* out);
NC_API nc_status nc_snac_halo(const nc_snac_config* cfg, nc_halo* out);

/* Per-handle chunk size, in latent frames, of nc_{dac,snac}_{encode,decode,from_codes}[_dev] and the DAC code-matrix pair:
 *   NC_CHUNK_AUTO (default)  one-shot whenever the one-shot call would be served (so every call that succeeds without this setting
 *                            issues exactly the same launches); chunked with a built-in chunk size only where the one-shot call
 *                            would be refused for size.  Decided before anything is launched.
 *   > 0                      every call with more frames than this runs chunked (rounded up to align)
 *   NC_CHUNK_OFF             never chunk: long clips return NC_EUNSUPPORTED
 * Chunked calls keep device memory independent of the clip length: the arena is sized by chunk + halos, and the host-pointer
 * entry points upload and download per chunk.  nc_snac_encode_tensor*, nc_snac_process_audio and the group calls are never chunked.
 * Encodec handles return NC_EUNSUPPORTED (48 kHz is segmented per second already; a window of the 24 kHz model does not stand for the clip
 * unless the LSTM's state is carried: live 24 kHz streams run through nc_encodec_causal_pool_*, "Encodec causal streams" below). */
#define NC_CHUNK_AUTO 0
#define NC_CHUNK_OFF (-1)
NC_API nc_status nc_codec_set_chunk_frames(nc_codec* h, int64_t chunk_frames);

/* What a call on `frames` latent frames (decode != 0: decode, else encode) would do under the handle's setting: n_chunks (1 = one
 * shot), the chunk size, the halos a window carries, and the activation-arena bytes the call needs. */
typedef struct nc_chunk_plan {
    int64_t n_chunks;
    int64_t chunk_frames;
    int64_t halo_left, halo_right;
    int64_t arena_bytes;
} nc_chunk_plan;
NC_API nc_status nc_codec_chunk_plan(const nc_codec* h, int32_t decode, int32_t B, int64_t frames, nc_chunk_plan* out);

/* --------------------------------------------------------------------------------- ragged batches
 * One call on B clips of UNEQUAL lengths (dataset tokenisation, Dia voice prompts, decoding generated code matrices).  Clip b's output
 * equals, bit for bit, the uniform call on that clip alone (B = 1); zero-padding the clips to the longest one would not (every layer pads
 * with zeros at its own edge, so a short clip inside a longer row sees biases and Snake outputs leak back into its last frames).
 * Layout: with the halos of the direction (halo_left / halo_right as nc_codec_chunk_plan reports them), a kept width C (a multiple of
 * align) and W = C + halo_left + halo_right,
 *   - a clip of F >= W frames is covered by windows of exactly W frames starting at min(j * C, F - W): the first is left-aligned and the
 *     last right-aligned to the clip, so both outer edges are true clip edges; every frame is kept by exactly one window and keeps clear
 *     of every interior window edge by the halo;
 *   - clips of F < W frames are not cut: clips of equal F form one group, a group is a batch of one-window clips of width F;
 *   - windows of all long clips run through the uniform launch sequences in batches of at most max_windows rows (as do the groups), so
 *     the activation arena is bounded by max_windows * W whatever B and the clip lengths.
 * Rows are gathered and kept columns scattered by table-driven kernels, one launch per tensor and batch.  Packed layouts: clip b's data
 * follows clip b-1's with no gap; lengths[] / frames[] are HOST arrays in both forms.  The *_dev forms take device pointers for the packed
 * tensors and enqueue on the handle's stream; the plain forms take host pointers, are synchronous, and stage the whole packed tensors on the
 * device.  NC_EINVAL for B <= 0, a length <= 0 or a null pointer; whatever status the uniform call on any one clip would return is returned
 * for the whole batch; every refusal is decided before anything is launched.
 * Not offered in ragged form: the z / latents / zq outputs, the DAC code-matrix pair (Dia's delayed matrices of unequal valid lengths
 * decode through nc_dia_decode_output, "Dia output stage" below), nc_snac_encode_tensor and the group calls.
 * Encodec clips are never cut into windows (48 kHz is segmented per second already; a window of a 24 kHz clip does not stand for the clip
 * unless the LSTM's state is carried, which "Encodec causal streams" below does for live streams): nc_codec_set_ragged_window / nc_codec_ragged_plan return NC_EUNSUPPORTED for Encodec handles.  Encodec
 * has ragged calls of its own that pool the SEGMENTS of all clips, nc_encodec_*_ragged below ("Encodec ragged batches"). */
typedef struct nc_ragged_plan {
    int64_t window_frames;     /* W */
    int64_t kept_frames;       /* C */
    int64_t halo_left, halo_right;
    int64_t n_windows;         /* windows of the clips with F >= W */
    int64_t n_window_batches;  /* launch batches they run in */
    int64_t n_exact_groups;    /* distinct F among the clips with F < W */
    int64_t n_rows;            /* n_windows + clips with F < W: entries of the window list */
    int64_t n_batches;         /* all launch batches (a group of more than max_windows clips is split) */
    int64_t arena_bytes;       /* activation arena: max_windows rows of W frames */
    int64_t total_frames;      /* sum of F_b */
    int64_t total_codes;       /* int64 codes of all clips with every codebook (DAC: n_codebooks * F_b; SNAC: sum_i F_b / vq_strides[i]) */
    int64_t total_samples;     /* decoded samples of all clips */
} nc_ragged_plan;
/* one row of a launch batch: frames [start, start + width) of `clip`, of which [keep_start, keep_start + keep_frames) are kept */
typedef struct nc_ragged_window {
    int32_t clip, batch;
    int64_t start, width;
    int64_t keep_start, keep_frames;
} nc_ragged_window;
/* The planner on a config alone (host functions: no handle, no device).  decode != 0: decode.  kept_frames / max_windows: 0 = the
 * defaults of nc_codec_set_ragged_window.  windows (nullable) receives the first `cap` rows in launch order. */
NC_API nc_status nc_dac_ragged_windows(const nc_dac_config* cfg, int32_t decode, int32_t B, const int64_t* frames, int64_t kept_frames,
                                       int32_t max_windows, nc_ragged_plan* out, nc_ragged_window* windows, int64_t cap);
NC_API nc_status nc_snac_ragged_windows(const nc_snac_config* cfg, int32_t decode, int32_t B, const int64_t* frames, int64_t kept_frames,
                                        int32_t max_windows, nc_ragged_plan* out, nc_ragged_window* windows, int64_t cap);
/* Per-handle kept width C (rounded up to align) and rows per launch batch; 0 selects the default, the best measured pair
 * (profiles/ragged_bench.json): 128 frames for DAC, 256 for SNAC, 128 rows. */
NC_API nc_status nc_codec_set_ragged_window(nc_codec* h, int64_t kept_frames, int32_t max_windows);
/* what a ragged call on these frame counts would do under the handle's setting */
NC_API nc_status nc_codec_ragged_plan(const nc_codec* h, int32_t decode, int32_t B, const int64_t* frames, nc_ragged_plan* out);

/* frames F_b and decoded samples of every clip (outputs nullable) */
NC_API nc_status nc_dac_ragged_query(const nc_codec* h, int32_t B, const int64_t* lengths, int64_t* frames, int64_t* decoded_lens);
/* pcm_packed [sum lengths] -> codes_packed: clip b as [n_q, F_b] row-major, clip after clip (sample_rate / n_q as nc_dac_encode) */
NC_API nc_status nc_dac_encode_ragged(nc_codec* h, const float* pcm_packed, int32_t B, const int64_t* lengths, int32_t sample_rate,
                                      int32_t n_q, int64_t* codes_packed);
NC_API nc_status nc_dac_encode_ragged_dev(nc_codec* h, const float* pcm_packed, int32_t B, const int64_t* lengths, int32_t sample_rate,
                                          int32_t n_q, int64_t* codes_packed);
/* FromCodes then Decode per window: codes_packed as above -> pcm_packed, clip b yields decoded_lens[b] samples */
NC_API nc_status nc_dac_decode_codes_ragged(nc_codec* h, const int64_t* codes_packed, int32_t B, const int64_t* frames, int32_t n_q,
                                            float* pcm_packed);
NC_API nc_status nc_dac_decode_codes_ragged_dev(nc_codec* h, const int64_t* codes_packed, int32_t B, const int64_t* frames, int32_t n_q,
                                                float* pcm_packed);
/* frames F_b (Preprocess pads), codes per clip and decoded samples of every clip (outputs nullable) */
NC_API nc_status nc_snac_ragged_query(const nc_codec* h, int32_t B, const int64_t* lengths, int64_t* frames, int64_t* codes_per_clip,
                                      int64_t* decoded_lens);
/* codes_packed: the levels of a clip side by side as in nc_snac_encode (codes_per_clip[b] values), clip after clip */
NC_API nc_status nc_snac_encode_ragged(nc_codec* h, const float* pcm_packed, int32_t B, const int64_t* lengths, int64_t* codes_packed);
NC_API nc_status nc_snac_encode_ragged_dev(nc_codec* h, const float* pcm_packed, int32_t B, const int64_t* lengths, int64_t* codes_packed);
/* noise: every clip's B = 1 noise block (nc_snac_noise_len(1, F_b) floats), clip after clip; NULL: clip b is drawn exactly as
 * nc_snac_decode(B = 1, seed + b) draws it */
NC_API nc_status nc_snac_decode_ragged(nc_codec* h, const int64_t* codes_packed, int32_t B, const int64_t* frames, const float* noise,
                                       uint64_t seed, float* pcm_packed);
NC_API nc_status nc_snac_decode_ragged_dev(nc_codec* h, const int64_t* codes_packed, int32_t B, const int64_t* frames, const float* noise,
                                           uint64_t seed, float* pcm_packed);

/* ---------------------------------------------------------------------------- incremental sessions
 * Codes or PCM pushed as they arrive (a text-to-speech model that emits code frames one at a time: Dia drives DAC, the Orpheus family
 * SNAC 24 kHz; a live capture that wants codes while it records).  A session keeps the history between calls, decides after every push
 * which outputs are final, and returns exactly those: the concatenated outputs of the pushes and the flush equal, bit for bit, what the
 * one-shot call on the whole sequence returns.
 * Contract.  With P frames pushed and E emitted so far, hl / hr the halos of the direction (halo_left / halo_right as
 * nc_codec_chunk_plan reports them) and align as in nc_halo:
 *   - a push emits the frames [E, floor_align(P - hr)); when that range is not empty it runs the window [max(0, E - hl), P) through the
 *     existing launch sequence and keeps that range.  A window that starts at 0 has the clip's true left edge, every other window edge
 *     is a cut edge, and every kept frame keeps clear of a cut edge by the halo;
 *   - the flush runs [max(0, E - hl), P), whose right edge is the clip's true end, and emits [E, P);
 *   - latency: an output is final hr frames after its own frame has arrived (the flush releases the rest); work per push of n frames:
 *     a window of hl + n + hr frames once the session is in steady state; resident history: at most hl + hr + align frames.
 * nc_session_schedule states the schedule as a host function (no handle, no device): one step per push, and one more for the flush
 * when flush != 0.  NC_EINVAL: a null pointer, n_pushes < 0, n_pushes == 0 with a flush (nothing to flush), a push that is not a
 * positive multiple of align. */
typedef struct nc_session_step {
    int64_t w0, w1;    /* the window the step runs, [w0, w1) in latent frames; w0 == w1: too little has arrived, nothing runs */
    int64_t k0, k1;    /* the frames it keeps, [k0, k1); k0 == k1: none */
    int64_t resident;  /* frames of history resident afterwards */
} nc_session_step;
NC_API nc_status nc_session_schedule(const nc_halo* halo, int32_t decode, int32_t n_pushes, const int64_t* push_frames, int32_t flush,
                                     nc_session_step* steps /* n_pushes + (flush != 0) entries */);

/* A session on a DAC or SNAC handle for B rows; decode != 0: codes in, PCM out, else PCM in, codes out.  n_q: the DAC codebooks a decode
 * session reads (0 = all; SNAC and encode sessions ignore it: an encode session writes every codebook).  Several sessions may live on one
 * handle: they share its arena and stream, and the caller serialises their calls like every other call on the handle.  A session
 * BORROWS its handle: destroy the sessions first.  Encodec handles return NC_EUNSUPPORTED: segmented Encodec models (48 kHz) stream through
 * nc_encodec_stream_pool_* below, causal models without segmentation (24 kHz) through nc_encodec_causal_pool_*, which carries the LSTM's
 * state ("Encodec causal streams").
 *   decode sessions  in: DAC codes [B, n_q, n]; SNAC every level at its own rate, [B, sum_i n / vq_strides[i]] as nc_snac_decode takes
 *                     them (n a multiple of align).  n_in = n frames.  out: PCM rows [B, out_cap], the first *n_out samples of a row valid.
 *                     SNAC with NoiseBlocks: `noise` holds the caller's noise for the pushed frames, one [B, 1, n * S_i] block per decoder
 *                     stage laid end to end (S_i = the product of the first i + 1 decoder rates); the session keeps the part that belongs
 *                     to the history, and the result equals nc_snac_decode on the noise concatenated along time.  noise == NULL: every push
 *                     draws its block on the device from (seed, frame position of the push) -- nc_session_set_seed, 0 by default.  This
 *                     is NOT the draw of nc_snac_decode(noise = NULL, seed): that draw's layout depends on the total length, which a
 *                     session does not know (the reference's own noise, torch.randn at inference, is not reproducible either).
 *   encode sessions   in: PCM rows [B, n], any n >= 1; n_in = n samples; `noise` is ignored.  Samples are buffered to whole hops (SNAC:
 *                     hop * align).  out: DAC codes rows [B, n_codebooks, out_cap], the first *n_out frames of a row valid; SNAC rows
 *                     [B, out_cap] holding the levels of the emitted frames side by side, coarse first (*n_out values in all).  The flush
 *                     writes +0.0f behind the last sample up to the codec's own padding, as the ragged calls do, and emits the rest.
 *                     There are no z / latents / zq outputs.
 * *n_out is the number of elements written per row.  It follows from frame counts alone and is known before anything is launched, so the
 * *_dev forms (device pointers, asynchronous on the handle's stream) never synchronise; the plain forms take host pointers and are
 * synchronous.  nc_session_query gives the out_cap a push of n_in needs (an upper bound over every state of the session; n_in == 0: what
 * a flush needs); out_cap is the row pitch of `out` in elements.  nc_session_pending: frames pushed and not yet emitted.
 * NC_EINVAL, decided before anything is launched: a null pointer, n_in <= 0, a decode push that is not a multiple of align, out_cap below
 * nc_session_query, a push or a second flush after a flush (until nc_session_reset, after which the session is as new), a flush with
 * nothing pushed.  NC_ESTATE without weights. */
typedef struct nc_session nc_session;
NC_API nc_status nc_session_create(nc_codec* h, int32_t decode, int32_t B, int32_t n_q, nc_session** out);
NC_API nc_status nc_session_destroy(nc_session* s);
NC_API nc_status nc_session_reset(nc_session* s);
NC_API nc_status nc_session_set_seed(nc_session* s, uint64_t seed);
NC_API nc_status nc_session_query(const nc_session* s, int64_t n_in, int64_t* out_cap);
NC_API nc_status nc_session_pending(const nc_session* s, int64_t* frames);
NC_API nc_status nc_session_push(nc_session* s, const void* in, int64_t n_in, const float* noise, void* out, int64_t out_cap, int64_t* n_out);
NC_API nc_status nc_session_push_dev(nc_session* s, const void* in, int64_t n_in, const float* noise, void* out, int64_t out_cap,
                                     int64_t* n_out);
NC_API nc_status nc_session_flush(nc_session* s, void* out, int64_t out_cap, int64_t* n_out);
NC_API nc_status nc_session_flush_dev(nc_session* s, void* out, int64_t out_cap, int64_t* n_out);

/* ---------------------------------------------------------------------------- session pool
 * n_slots independent streams on one DAC or SNAC handle, one direction, stepped together (a server with many users whose streams begin,
 * push and end at different times).  Every slot is a B = 1 session with its own schedule state; one step advances any subset of slots,
 * each by its own amount, and every slot's output is, bit for bit, what a B = 1 nc_session returns for the same sequence of pushes
 * (DESIGN.md 4g).  Entries whose step runs a window are grouped by the window's width in frames; a group runs as one uniform batch
 * through the existing launch sequence (at most the handle's ragged max_windows rows per batch, nc_codec_set_ragged_window).
 * A step is n entries (slots[i], n_in[i]): n_in > 0 pushes that many frames (decode) or samples (encode), n_in == 0 flushes the slot; a
 * slot appears at most once.  Inputs are packed in entry order: DAC decode codes [n_q, n_in] per entry (n_q fixed at creation; 0 = all),
 * SNAC decode the levels of the entry side by side, encode the PCM samples; a flush contributes nothing.  noise_packed (SNAC decode
 * with NoiseBlocks): per pushing entry, stage after stage, as nc_session_push takes it for B = 1; NULL: every pushing entry draws its
 * block from (the slot's seed, the slot's frame position) exactly as a session with that seed does.  Outputs are packed entry after
 * entry: decode [n_out[i]] samples; DAC encode [n_codebooks, n_out[i]]; SNAC encode the n_out[i] values of the emitted frames, levels
 * side by side.  n_out[i] is host arithmetic: nc_session_pool_query returns the exact n_out of every entry for the pool's current
 * state, so the packed output can be sized before the step; out_cap is the capacity of out_packed in elements.  The *_dev form takes
 * device pointers and is asynchronous on the handle's stream; the plain form takes host pointers and is synchronous.
 * The whole call is validated before anything is launched and before any slot changes -- NC_EINVAL: a null pointer, n <= 0, a slot out
 * of range or named twice, n_in < 0, a decode push that is not a multiple of align, a push or flush of a flushed slot (until
 * nc_session_pool_reset_slot), a flush of a slot with nothing pushed, out_cap below the sum the query gives; NC_ESTATE without weights;
 * NC_EUNSUPPORTED for Encodec handles.  A refused step leaves every slot as it was.  A pool BORROWS its handle: destroy it first.
 * nc_session_pool_plan states the grouping as a host function (no handle, no device): stream i has pushed[i] / emitted[i] frames and
 * pushes push_frames[i] more (0: flush); steps[i] is its step as nc_session_schedule reports it, group_of[i] the batch its window runs
 * in (-1: no window), batches numbered narrowest window first; no batch has more than max_rows rows (0 = the default, 128). */
typedef struct nc_session_pool nc_session_pool;
NC_API nc_status nc_session_pool_plan(const nc_halo* halo, int32_t decode, int32_t n, const int64_t* pushed, const int64_t* emitted,
                                      const int64_t* push_frames, int32_t max_rows, nc_session_step* steps, int32_t* group_of,
                                      int32_t* n_groups);
NC_API nc_status nc_session_pool_create(nc_codec* h, int32_t decode, int32_t n_slots, int32_t n_q, nc_session_pool** out);
NC_API nc_status nc_session_pool_destroy(nc_session_pool* p);
NC_API nc_status nc_session_pool_reset_slot(nc_session_pool* p, int32_t slot);
NC_API nc_status nc_session_pool_set_seed(nc_session_pool* p, int32_t slot, uint64_t seed);
NC_API nc_status nc_session_pool_pending(const nc_session_pool* p, int32_t slot, int64_t* frames);
NC_API nc_status nc_session_pool_query(const nc_session_pool* p, int32_t n, const int32_t* slots, const int64_t* n_in, int64_t* n_out);
NC_API nc_status nc_session_pool_step(nc_session_pool* p, int32_t n, const int32_t* slots, const int64_t* n_in, const void* in_packed,
                                      const float* noise_packed, void* out_packed, int64_t out_cap, int64_t* n_out);
NC_API nc_status nc_session_pool_step_dev(nc_session_pool* p, int32_t n, const int32_t* slots, const int64_t* n_in, const void* in_packed,
                                          const float* noise_packed, void* out_packed, int64_t out_cap, int64_t* n_out);

/* -------------------------------------------------------------------------------------- Encodec
 * replaces: new Encodec(EncodecConfig)            NeuralCodecs.Torch/Models/Encodec.cs:46-90
 * Only channels / dimension / norm / causal reach SEANet in the reference (Encodec.cs:57-68, deviation D11); the other SEANet
 * fields are its hard defaults (SEANetEncoder.cs:37-56) and are carried here so reduced-width test models can be built. */
typedef struct {
    int32_t sample_rate;        /* 24000 | 48000 */
    int32_t channels;           /* 1 | 2 */
    int32_t dimension;          /* 128 (HiddenSize == CodebookDim) */
    int32_t n_filters;          /* 32 */
    int32_t n_ratios;           /* 4 */
    int32_t ratios[8];          /* 8,5,4,2 (decoder order; the encoder runs them reversed) */
    int32_t lstm_layers;        /* 2 */
    int32_t compress;           /* 2 */
    int32_t kernel_size;        /* 7 */
    int32_t last_kernel_size;   /* 7 */
    int32_t residual_kernel_size; /* 3 */
    int32_t time_group_norm;    /* 0: weight_norm (24 kHz), 1: GroupNorm(1,C) after every conv (48 kHz) */
    int32_t causal;             /* 24 kHz: 1 */
    int32_t normalize;          /* 48 kHz: 1 (per-frame RMS scale) */
    int32_t segment_length;     /* samples; 0 = no segmentation (24 kHz); 48 kHz: 48000 */
    int32_t segment_stride;     /* samples; 48 kHz: 47520 (1 % overlap) */
    int32_t codebook_size;      /* 1024 */
    int32_t n_codebooks;        /* quantizer layers built: 1000*max(bandwidths)/(frame_rate*10) (Encodec.cs:70-71): 32 | 16 */
    int32_t frame_rate;         /* ceil(sample_rate / hop) */
    float bandwidth;            /* target kbps -> n_q = max(1, floor(bandwidth*1000 / (log2(codebook_size)*frame_rate))) */
} nc_encodec_config;

NC_API nc_status nc_encodec_create(const nc_encodec_config* cfg, int device_index, nc_codec** out);
/* replaces: Encodec.SetTargetBandwidth(float)      Models/Encodec.cs:409-419 (the caller validates membership in TargetBandwidths) */
NC_API nc_status nc_encodec_set_bandwidth(nc_codec* h, float bandwidth_kbps);

/* Frame layout of Encodec.Encode for clips of T samples: number of EncodedFrames (segments), codebooks in use n_q, frames T'_f of
 * every segment (frame_lens has room for `cap` entries), decoded length of Decode (before forward()'s trim to T). */
NC_API nc_status nc_encodec_query(const nc_codec* h, int64_t T, int32_t* n_frames, int32_t* n_q, int64_t* frame_lens, int32_t cap,
                                  int64_t* decoded_len);
/* The reference's Decode(List<EncodedFrame>) takes no clip length (Models/Encodec.cs:213-235: the frames alone fix the output,
 * (n-1)*stride + decoded(last frame)).  This gives the smallest clip length T whose segment layout is exactly `n_frames` segments
 * with frame_lens[i] code frames in segment i (with overlapping segments the last TWO can be short) -- the T to hand to
 * nc_encodec_decode for such a list.  NC_EINVAL when no clip length produces that layout. */
NC_API nc_status nc_encodec_clip_length(const nc_codec* h, int32_t n_frames, const int64_t* frame_lens, int64_t* T);

/* replaces: Encodec.Encode(Tensor x[B,C,T]) -> List<EncodedFrame>     Models/Encodec.cs:259-285, EncodeFrame :457-489
 *   codes  int64: the EncodedFrame.Codes tensors [B,n_q,T'_f] laid end to end in segment order
 *   scales float32 [n_frames,B] (EncodedFrame.Scale; written only when normalize) -- nullable otherwise
 *   emb    nullable: encoder outputs [B,dimension,T'_f] end to end (test hook) */
NC_API nc_status nc_encodec_encode(nc_codec* h, const float* pcm, int32_t B, int64_t T, int64_t* codes, float* scales, float* emb);
NC_API nc_status nc_encodec_encode_dev(nc_codec* h, const float* pcm, int32_t B, int64_t T, int64_t* codes, float* scales, float* emb);

/* replaces: Encodec.Decode(List<EncodedFrame>) -> [B,C,decoded_len]    Models/Encodec.cs:213-235, DecodeFrame :436-455,
 * DSP.LinearOverlapAdd AudioTools/AudioTensorDSP.cs:161-261.  T is the clip length the frames were encoded from (it fixes the
 * segment layout); n_q the number of codebooks present in `codes`. */
NC_API nc_status nc_encodec_decode(nc_codec* h, const int64_t* codes, const float* scales, int32_t B, int64_t T, int32_t n_q, float* pcm);
NC_API nc_status nc_encodec_decode_dev(nc_codec* h, const int64_t* codes, const float* scales, int32_t B, int64_t T, int32_t n_q,
                                       float* pcm);

/* ----------------------------------------------------------------------- Encodec ragged batches
 * One call on B clips of UNEQUAL lengths (whole files: Examples/Program.cs:293-322, EncodecCompressor).  The reference cuts every clip
 * into segments, and a segment depends on nothing outside itself (GroupNorm(1,C), the RMS scale, the LSTM state and the RVQ are all per
 * sample), so the segments of ALL clips are rows of uniform batches: nothing is recomputed and no halo is needed.  Clip b's output equals,
 * bit for bit, the one-clip call (B = 1) on that clip.
 *   - a row is one (clip, segment) pair of the clip's segment list; its key is the segment's sample count for Encode and its code-frame
 *     count for Decode;
 *   - rows of equal key, from any clips, run through the unchanged launch sequences in batches of at most max_rows rows (keys in
 *     descending order, rows of a key segment-major then by clip: for equal lengths this is the uniform call's grouping);
 *   - models without segmentation (segment_length == 0: the 24 kHz preset) have one row per clip whose key is the clip's own length, so
 *     only clips of EQUAL length share a batch -- the LSTM runs over the whole clip and no part of it stands for the clip;
 *   - the activation arena is bounded by max_rows rows of one segment (without segmentation: of the longest clip), whatever B is.
 * Packed layouts, clip after clip with no gap: clip b's PCM is [channels, lengths[b]] (Decode: [channels, decoded_lens[b]]); its codes
 * are exactly the `codes` buffer of nc_encodec_encode(B = 1) on that clip (its frames [n_q, T'_f] end to end), its scales its
 * n_frames[b] floats, its emb (nullable test hook) its frames [dimension, T'_f] end to end.  lengths[] is a HOST array of clip lengths
 * in samples in both forms and both directions.  The *_dev forms take device pointers for the packed tensors and enqueue on the handle's
 * stream; the plain forms take host pointers and are synchronous.  NC_EINVAL for B <= 0, a null pointer or a length <= 0; whatever the
 * one-clip call would answer for any clip (a clip too short for the residual blocks, for instance) is the answer for the whole batch, names
 * the clip index, and is decided before anything is launched. */
typedef struct nc_encodec_ragged_plan {
    int64_t n_rows;             /* (clip, segment) pairs */
    int64_t n_keys;             /* distinct keys */
    int64_t n_batches;          /* launch batches: sum over the keys of ceil(rows of the key / max_rows) */
    int64_t max_rows;           /* rows per launch batch in force */
    int64_t total_code_frames;  /* sum of T'_f over all rows */
    int64_t total_codes;        /* int64 values of codes_packed: n_q * total_code_frames (n_q from the config's / handle's bandwidth) */
    int64_t total_scales;       /* floats of scales_packed: n_rows */
    int64_t total_samples;      /* floats per channel of the decoded pcm_packed: sum of decoded_lens[b] */
} nc_encodec_ragged_plan;
/* one row: segment `segment` of clip `clip` is row `row` of launch batch `batch`; it starts `offset` samples into the clip, holds
 * `length` samples (decode != 0: the samples its frame decodes to) and `frames` code frames */
typedef struct nc_encodec_ragged_row {
    int32_t clip, segment, batch, row;
    int64_t offset, length, frames;
} nc_encodec_ragged_row;
/* The planner on a config alone (host function: no handle, no device).  decode != 0: decode.  max_rows: 0 = the default, at most 4096.
 * rows (nullable) receives the first `cap` rows in launch order. */
NC_API nc_status nc_encodec_ragged_rows(const nc_encodec_config* cfg, int32_t decode, int32_t B, const int64_t* lengths, int32_t max_rows,
                                        nc_encodec_ragged_plan* out, nc_encodec_ragged_row* rows, int64_t cap);
/* Per-handle rows per launch batch; 0 selects the default, the best measured value (profiles/encodec_ragged_bench.json) */
NC_API nc_status nc_encodec_set_ragged_rows(nc_codec* h, int32_t max_rows);
/* what a ragged call on these clip lengths would do under the handle's setting and bandwidth (rows nullable, as above) */
NC_API nc_status nc_encodec_ragged_rows_of(const nc_codec* h, int32_t decode, int32_t B, const int64_t* lengths, nc_encodec_ragged_plan* out,
                                           nc_encodec_ragged_row* rows, int64_t cap);
/* per clip (outputs nullable): segments, code frames summed over them, decoded samples -- the sums of nc_encodec_query on every clip */
NC_API nc_status nc_encodec_ragged_query(const nc_codec* h, int32_t B, const int64_t* lengths, int32_t* n_frames, int64_t* code_frames,
                                         int64_t* decoded_lens);
NC_API nc_status nc_encodec_encode_ragged(nc_codec* h, const float* pcm_packed, int32_t B, const int64_t* lengths, int64_t* codes_packed,
                                          float* scales_packed, float* emb_packed);
NC_API nc_status nc_encodec_encode_ragged_dev(nc_codec* h, const float* pcm_packed, int32_t B, const int64_t* lengths, int64_t* codes_packed,
                                              float* scales_packed, float* emb_packed);
NC_API nc_status nc_encodec_decode_ragged(nc_codec* h, const int64_t* codes_packed, const float* scales_packed, int32_t B,
                                          const int64_t* lengths, int32_t n_q, float* pcm_packed);
NC_API nc_status nc_encodec_decode_ragged_dev(nc_codec* h, const int64_t* codes_packed, const float* scales_packed, int32_t B,
                                              const int64_t* lengths, int32_t n_q, float* pcm_packed);

/* ------------------------------------------------------------------------- Encodec stream pool
 * replaces: Encodec.Encode / Encodec.Decode (Models/Encodec.cs:259-285, 213-235) and DSP.LinearOverlapAdd (AudioTools/AudioTensorDSP.cs:
 * 161-261) for a caller whose PCM or frames ARRIVE over time.  Segmented models only (segment_length > 0: the 48 kHz preset): a segment
 * depends on nothing outside itself, so a stream is encoded segment by segment as its samples arrive and decoded frame by frame, and what
 * a slot emits, laid end to end, is bit for bit what nc_encodec_encode / nc_encodec_decode (B = 1) give on the whole stream.
 * The latency is one segment, by the codec's own design.  A model without segmentation (the 24 kHz preset: its LSTM runs over the whole
 * clip) answers NC_EUNSUPPORTED at create.
 * A pool is n_slots independent streams of `channels` channels on one handle, one direction; the one-stream session is a pool with one
 * slot.  A step is n entries (slots[i], n_in[i], flush[i]) naming distinct slots (flush == NULL: nobody flushes).  Rows of equal key
 * (Encode: samples, Decode: code frames) from any slots run through the unchanged launch sequences in batches of at most the handle's
 * ragged max_rows (nc_encodec_set_ragged_rows), keys in descending order: a lock-step step of n streams is one n-row launch sequence.
 *   encode pool (decode == 0)   an entry pushes n_in >= 0 samples, [channels, n_in], packed entry after entry in in_packed.  A stream
 *       that has received T_s samples has emitted, once each and in order, every segment k with k * stride + segment_length <= T_s; the
 *       samples from the next segment's start on (fewer than segment_length) stay in the slot; a push that completes no segment only
 *       appends.  flush != 0 (after the entry's last n_in samples) emits the remaining segments of the T_s-sample clip -- up to two short
 *       ones -- and ends the slot until nc_encodec_stream_pool_reset_slot.  Every emitted segment comes as nc_encodec_encode(B = 1) lays
 *       it out: out_packed int64 codes [n_q, T'_f] end to end (n_q: the handle's bandwidth), scales_out one float per segment (written
 *       when the model normalises; nullable), emb_packed (nullable test hook) [dimension, T'_f] end to end; entry after entry.
 *       scales_in and frame_lens are ignored.
 *   decode pool (decode != 0; n_q fixed at create, 0 = the handle's bandwidth)   an entry pushes n_in >= 0 frames: in_packed their int64
 *       codes [n_q, F] end to end, scales_in one float per frame (models that normalise), entry after entry.  frame_lens (HOST array,
 *       nullable) holds F of every frame of every entry in the same order; NULL: every frame is a full segment's F_full.  Without a flush
 *       every frame must be F_full long and the entry emits [channels, n_in * stride] samples: after frames 0..k the samples
 *       [0, (k + 1) * stride) are final.  A flush entry's frames may end in the one or two short frames of the clip's tail; the whole
 *       list is validated as nc_encodec_clip_length validates a layout, the entry emits the rest and the slot is ended.  out_packed:
 *       float [channels, n_out[i]] entry after entry.  scales_out and emb_packed are ignored.
 * n_frames[i] (nullable): segments emitted | frames consumed; n_out[i] (nullable): code frames emitted | samples per channel emitted.
 * Both are host arithmetic: nc_encodec_stream_pool_query gives them for the pool's current state (n_samples: Decode the samples per
 * channel the entry emits, Encode the samples the slot keeps afterwards), so out_packed can be sized first; out_cap is its capacity in
 * elements (Encode: n_q * the code frames of all entries; Decode: channels * the samples of all entries).  The *_dev form takes device
 * pointers for the packed tensors, host arrays for slots / n_in / flush / frame_lens, and enqueues on the handle's stream; the plain
 * form takes host pointers and is synchronous.  nc_encodec_stream_pool_pending: Encode the samples the slot holds, Decode the decoded
 * samples per channel not yet emitted.
 * Everything is decided before anything is launched, names the slot, and leaves every slot as it was -- NC_EINVAL: a null pointer,
 * n <= 0, a slot out of range or named twice, n_in < 0, a push to an ended slot, a flush of a slot that has received nothing, a decode
 * push whose frame is not F_full long, tail frames that no clip length produces, out_cap below the query, and whatever the one-clip
 * call answers for a tail segment (one too short for the residual blocks, for instance); NC_ESTATE without weights.  A pool BORROWS its
 * handle: destroy it first; the caller serialises its calls with every other call on the handle.
 * nc_encodec_stream_plan states a step as a host function (no handle, no device), like nc_encodec_ragged_rows: stream i has received
 * pushed[i] samples (Decode: frames) and emitted emitted[i] segments (Decode: samples per channel) and now brings n_in[i] / flush[i] /
 * frame_lens; rows (nullable, the first `cap`) are the rows that would run, in launch order, `clip` being the stream's index i and
 * `offset` the segment's first sample in the stream; n_frames / code_frames / n_samples (nullable) as the query gives them. */
typedef struct nc_encodec_stream_pool nc_encodec_stream_pool;
NC_API nc_status nc_encodec_stream_plan(const nc_encodec_config* cfg, int32_t decode, int32_t n, const int64_t* pushed, const int64_t* emitted,
                                        const int64_t* n_in, const int32_t* flush, const int64_t* frame_lens, int32_t max_rows,
                                        nc_encodec_ragged_plan* out, nc_encodec_ragged_row* rows, int64_t cap, int32_t* n_frames,
                                        int64_t* code_frames, int64_t* n_samples);
NC_API nc_status nc_encodec_stream_pool_create(nc_codec* h, int32_t decode, int32_t n_slots, int32_t n_q, nc_encodec_stream_pool** out);
NC_API nc_status nc_encodec_stream_pool_destroy(nc_encodec_stream_pool* p);
NC_API nc_status nc_encodec_stream_pool_reset_slot(nc_encodec_stream_pool* p, int32_t slot);
NC_API nc_status nc_encodec_stream_pool_pending(const nc_encodec_stream_pool* p, int32_t slot, int64_t* n);
NC_API nc_status nc_encodec_stream_pool_query(const nc_encodec_stream_pool* p, int32_t n, const int32_t* slots, const int64_t* n_in,
                                              const int32_t* flush, const int64_t* frame_lens, int32_t* n_frames, int64_t* code_frames,
                                              int64_t* n_samples);
/* the rows the step would run under the pool's current state and the handle's max_rows, as nc_encodec_stream_plan reports them (`clip`:
 * the entry's index; rows nullable, the first `cap` in launch order): per entry its segments with their code frames */
NC_API nc_status nc_encodec_stream_pool_plan(const nc_encodec_stream_pool* p, int32_t n, const int32_t* slots, const int64_t* n_in,
                                             const int32_t* flush, const int64_t* frame_lens, nc_encodec_ragged_plan* out,
                                             nc_encodec_ragged_row* rows, int64_t cap);
NC_API nc_status nc_encodec_stream_pool_step(nc_encodec_stream_pool* p, int32_t n, const int32_t* slots, const int64_t* n_in,
                                             const int32_t* flush, const int64_t* frame_lens, const void* in_packed, const float* scales_in,
                                             void* out_packed, float* scales_out, float* emb_packed, int64_t out_cap, int32_t* n_frames,
                                             int64_t* n_out);
NC_API nc_status nc_encodec_stream_pool_step_dev(nc_encodec_stream_pool* p, int32_t n, const int32_t* slots, const int64_t* n_in,
                                                 const int32_t* flush, const int64_t* frame_lens, const void* in_packed,
                                                 const float* scales_in, void* out_packed, float* scales_out, float* emb_packed,
                                                 int64_t out_cap, int32_t* n_frames, int64_t* n_out);

/* ------------------------------------------------------------------------- Encodec causal streams
 * replaces: Encodec.Encode / Encodec.Decode (Models/Encodec.cs:259-285, 213-235) with SLSTM.forward (Modules/Encodec/SLSTM.cs:40-57) carried
 * across calls, for a caller whose PCM or code frames ARRIVE over time on a CAUSAL model without segmentation (the 24 kHz preset).  With
 * causal == 1 no operator looks to the right (SConv1d pads on the left, SConvTranspose1d trims on the right, the SLSTM is
 * unidirectional), so a stream that carries the LSTM's (h, c) forward never recomputes its past: what a slot emits, laid end to end, is
 * bit for bit what nc_encodec_encode / nc_encodec_decode (B = 1) give on the whole stream -- codes, the emb hook and PCM.
 * Admitted: causal != 0, segment_length == 0, normalize == 0, time_group_norm == 0; anything else answers NC_EUNSUPPORTED at create and
 * names the condition.  Segmented models stream through nc_encodec_stream_pool_* above.
 * hop = the product of the ratios.  A pool is n_slots independent streams on one handle, one direction; a step is n entries
 * (slots[i], n_in[i], flush[i]) naming distinct slots (flush == NULL: nobody flushes).
 *   encode pool (decode == 0)   an entry pushes n_in >= 0 samples, [channels, n_in], packed entry after entry in in_packed.  A stream
 *       that has received T_s samples has emitted frames 0 .. floor(T_s / hop) - 1 once it holds min_frames_e frames (below that a push
 *       only appends: the one-clip call's left reflect pad reads the first kernel_size - 1 samples and frames).  A step runs the
 *       convolutional front on the window that starts halo_e frames before the first new frame (clamped to 0) and drops its first
 *       halo_e frames, the LSTM on the new frames from the slot's (h, c), the last convolution on the carried last_kernel_size - 1 LSTM
 *       frames + the new ones, the quantizer on the new frames.  flush != 0 runs the window up to the stream's true end (its right
 *       reflect pad is then the one-clip call's), emits the remaining frames and ends the slot until ..._reset_slot; a stream flushed
 *       below min_frames_e runs as the one-clip call on what it holds and answers what that call answers.  out_packed: int64 codes
 *       [n_q, n_out[i]] entry after entry (n_q: the handle's bandwidth); emb_packed (nullable test hook): [dimension, n_out[i]].
 *   decode pool (decode != 0; n_q fixed at create, 0 = the handle's bandwidth)   an entry pushes n_in >= 0 code frames: in_packed int64
 *       [n_q, n_in] entry after entry.  Frames are held until the stream has min_frames_d of them; from then on a push of n frames emits
 *       [channels, n * hop] samples -- after frames 0..k the samples [0, (k + 1) * hop) are final: no latency.  flush emits what is held
 *       (as the one-clip call where the stream is shorter than min_frames_d) and ends the slot.  out_packed: float [channels, n_out[i]].
 * Rows whose window width and number of new frames are equal run as one batch of at most the handle's ragged max_rows rows
 * (nc_encodec_set_ragged_rows) through the unchanged launch sequences, keys in descending order: a lock-step step of n streams is one
 * n-row launch sequence.  n_out[i] (nullable): code frames | samples per channel the entry emits; nc_encodec_causal_pool_query gives
 * them beforehand.  out_cap: capacity of out_packed in elements (n_q * frames | channels * samples of all entries).  The *_dev form takes
 * device pointers for the packed tensors and enqueues on the handle's stream; the plain form takes host pointers and is synchronous.
 * nc_encodec_causal_pool_pending: Encode the samples received that no emitted frame covers, Decode the frames held and not yet decoded.
 * Everything is decided before anything is launched, names the slot, and leaves every slot as it was -- NC_EINVAL: a null pointer,
 * n <= 0, a slot out of range or named twice, n_in < 0, a push to an ended slot, a flush of a slot that has received nothing, out_cap
 * below the query; NC_ESTATE without weights.  That guarantee covers the refusals, which are all decided at plan time; a step that fails
 * AFTER its launches began (a HIP error, NC_EDEVICE) has already written the named slots' device state, so those slots are ended and take
 * no push until nc_encodec_causal_pool_reset_slot; slots the step did not name are untouched.  A pool BORROWS its handle: destroy it first.
 * nc_encodec_causal_plan is a host function (no handle, no device): stream i has received received[i] samples (Decode: frames) and
 * emitted emitted[i] frames (Decode: decoded that many frames) and now brings n_in[i] / flush[i].  info (nullable): the halos and minimum
 * windows of the config; rows (nullable, the first `cap`, in launch order): the windows that would run; n_out as above. */
typedef struct nc_encodec_causal_info {
    int64_t hop;
    int64_t halo_e;         /* frames of the encoder front recomputed and dropped in front of the new ones */
    int64_t halo_d;         /* LSTM-output frames the decoder's up-stack recomputes in front of the new ones */
    int64_t min_frames_e;   /* frames a stream must hold before its first emission (encode) */
    int64_t min_frames_d;   /* ... (decode) */
    int64_t carry_e;        /* LSTM-output frames the encode slot carries: last_kernel_size - 1 */
    int64_t carry_d;        /* code frames the decode slot carries: max(kernel_size - 1, min_frames_d - 1) */
    int64_t taint_e;        /* samples-deep dependency model: frames at the LSTM input a window's left edge can reach (halo_e before the
                               minimum-window rule is applied) */
    int64_t taint_d;        /* decoded samples a window's left edge can reach (halo_d = ceil(taint_d / hop)) */
} nc_encodec_causal_info;
typedef struct nc_encodec_causal_row {
    int32_t entry;          /* index of the entry (plan: of the stream) */
    int32_t batch;          /* launch batch, in launch order */
    int32_t row;            /* row within the batch */
    int32_t one_clip;       /* 1: a stream flushed below the minimum, run as the one-clip call */
    int64_t start;          /* first sample (Decode: first code frame) of the window in the stream */
    int64_t width;          /* samples (Decode: code frames) of the window */
    int64_t new_frames;     /* frames the row emits (Decode: frames it decodes) */
} nc_encodec_causal_row;
typedef struct nc_encodec_causal_pool nc_encodec_causal_pool;
NC_API nc_status nc_encodec_causal_plan(const nc_encodec_config* cfg, int32_t decode, int32_t n, const int64_t* received, const int64_t* emitted,
                                        const int64_t* n_in, const int32_t* flush, int32_t max_rows, nc_encodec_causal_info* info,
                                        nc_encodec_causal_row* rows, int64_t cap, int64_t* n_rows, int64_t* n_batches, int64_t* n_out);
NC_API nc_status nc_encodec_causal_pool_create(nc_codec* h, int32_t decode, int32_t n_slots, int32_t n_q, nc_encodec_causal_pool** out);
NC_API nc_status nc_encodec_causal_pool_destroy(nc_encodec_causal_pool* p);
NC_API nc_status nc_encodec_causal_pool_reset_slot(nc_encodec_causal_pool* p, int32_t slot);
NC_API nc_status nc_encodec_causal_pool_pending(const nc_encodec_causal_pool* p, int32_t slot, int64_t* n);
NC_API nc_status nc_encodec_causal_pool_query(const nc_encodec_causal_pool* p, int32_t n, const int32_t* slots, const int64_t* n_in,
                                              const int32_t* flush, int64_t* n_out);
NC_API nc_status nc_encodec_causal_pool_plan(const nc_encodec_causal_pool* p, int32_t n, const int32_t* slots, const int64_t* n_in,
                                             const int32_t* flush, nc_encodec_causal_row* rows, int64_t cap, int64_t* n_rows,
                                             int64_t* n_batches);
NC_API nc_status nc_encodec_causal_pool_step(nc_encodec_causal_pool* p, int32_t n, const int32_t* slots, const int64_t* n_in,
                                             const int32_t* flush, const void* in_packed, void* out_packed, float* emb_packed,
                                             int64_t out_cap, int64_t* n_out);
NC_API nc_status nc_encodec_causal_pool_step_dev(nc_encodec_causal_pool* p, int32_t n, const int32_t* slots, const int64_t* n_in,
                                                 const int32_t* flush, const void* in_packed, void* out_packed, float* emb_packed,
                                                 int64_t out_cap, int64_t* n_out);

/* ------------------------------------------------------------------------------- code containers
 * Device-side bit packing of code tensors: the wire layout of the reference's BitPacker / BitUnpacker
 * (Modules/Encodec/BitPacker.cs: values LSB-first into a little-endian bit stream, `bits` per value, flushed to a whole byte) in the
 * order EncodecCompressor writes a frame (EncodecCompressor.cs:170-181: t outer, codebook k inner).  One packed row per clip.
 *   codes  [B,K,T] int64 (device)         packed [B, nc_packed_bytes(K*T, bits)] uint8 (device)
 * Used for `.ecdc` payloads without the language model and to shrink the multi-GPU code all-gather 64/bits times.
 * Only the low `bits` bits of a code are written: where BitPacker.Push throws ArgumentOutOfRangeException (a negative code, a code of
 * 1 << bits or more) these calls cannot, so the caller checks the range (the Python mirror does); the neighbours' bits are never
 * touched.  The pad bits of a row's last byte are written as 0 and ignored when unpacking.  `packed` may have any byte alignment.
 * 1 <= bits <= 24; B, K, T > 0; NULL pointers and a device index out of range: NC_EINVAL, nothing written. */
NC_API int64_t nc_packed_bytes(int64_t n_values, int32_t bits);
NC_API nc_status nc_pack_codes_dev(int device_index, const int64_t* codes, int32_t B, int32_t K, int64_t T, int32_t bits, uint8_t* packed,
                                   void* hip_stream);
NC_API nc_status nc_unpack_codes_dev(int device_index, const uint8_t* packed, int32_t B, int32_t K, int64_t T, int32_t bits,
                                     int64_t* codes, void* hip_stream);
/* host-pointer, synchronous variants */
NC_API nc_status nc_pack_codes(int device_index, const int64_t* codes, int32_t B, int32_t K, int64_t T, int32_t bits, uint8_t* packed);
NC_API nc_status nc_unpack_codes(int device_index, const uint8_t* packed, int32_t B, int32_t K, int64_t T, int32_t bits, int64_t* codes);

/* ------------------------------------------------------------------------------- audio pre / post
 * The host-side steps either side of the tensor path as device kernels, so a float[]-level caller can keep its
 * audio in HBM from the decoded WAV bytes to the codec and back.  Device pointers, asynchronous on `hip_stream` (NULL = null
 * stream).  Arithmetic follows the reference statement by statement (bit-identical results):
 *   pcm16_to_float   replaces AudioUtils.AudioBytesToFloatArray (Core/Utils/AudioUtils.cs:13-36): out = int16 * (1/32768f), same
 *                    order; planar != 0 writes channel-major [channels][n_frames] like NAudioUtils.cs:94-104 / Examples/Program.cs:391-401
 *   float_to_pcm16   replaces AudioUtils.FloatArrayToAudioBytes (AudioUtils.cs:172-186) with the clamp of Dia.SaveAudio
 *                    (Models/Dia.cs:918-923): (short)(clamp(x,-1,1) * 32767), truncating.  A NaN sample gives 0, as Math.Min / Math.Max
 *                    keep the NaN and (short)NaN is 0 (never full scale); +-inf gives +-32767, -0.0 gives 0
 *   mix_to_mono      replaces AudioUtils.ConvertToMono (AudioUtils.cs:45-61): interleaved [n_frames][channels] -> [n_frames]
 *   interleave       replaces AudioUtils.DeinterleaveToInterleave (AudioUtils.cs:90-101), any channel count
 *   deinterleave     replaces AudioUtils.InterleaveToDeinterleave (AudioUtils.cs:204-219)
 *   resample_linear  replaces AudioUtils.ResampleLinear (AudioUtils.cs:329-354) == SNAC.ResampleAudio (Models/SNAC.cs:284-308):
 *                    [B][n_in] -> [B][nc_audio_resample_len(n_in, src, dst)], binary64 position arithmetic
 * nc_audio_resample_len is (int)(n_in * ((double)dst / src)) with the product in binary64.  It returns -1 for n_in < 0, a rate <= 0, or
 * a product of 2^31 or more (the reference's (int) goes negative there and its `new float[n]` throws); nc_audio_resample_linear_dev
 * refuses those, and a length of 0, with NC_EINVAL before anything is launched. */
NC_API int64_t nc_audio_resample_len(int64_t n_in, int32_t src_rate, int32_t dst_rate);
NC_API nc_status nc_audio_pcm16_to_float_dev(int device_index, const int16_t* pcm, int64_t n_frames, int32_t channels, int32_t planar,
                                             float* out, void* hip_stream);
NC_API nc_status nc_audio_float_to_pcm16_dev(int device_index, const float* in, int64_t n, int16_t* out, void* hip_stream);
NC_API nc_status nc_audio_mix_to_mono_dev(int device_index, const float* in, int64_t n_frames, int32_t channels, float* out, void* hip_stream);
NC_API nc_status nc_audio_interleave_dev(int device_index, const float* planar, int64_t n_frames, int32_t channels, float* out,
                                         void* hip_stream);
NC_API nc_status nc_audio_deinterleave_dev(int device_index, const float* interleaved, int64_t n_frames, int32_t channels, float* out,
                                           void* hip_stream);
NC_API nc_status nc_audio_resample_linear_dev(int device_index, const float* in, int32_t B, int64_t n_in, int32_t src_rate, int32_t dst_rate,
                                              float* out, void* hip_stream);

/* -------------------------------------------------------------------------------------- Dia output stage
 * What Dia runs between its language model and DAC, and behind DAC, as device kernels (csrc/nc_dia.hip): a batch of
 * generations stays in HBM from the delayed codes to the waveforms and decodes as ONE ragged batch instead of B single-clip decodes.
 *   codes_delayed  int64 [B, T_gen, C], Dia's layout (C fastest); C = the model's n_codebooks, at most 32
 *   delay[]        C non-negative steps (DataConfig.DelayPattern), maxd = max(delay); T_gen > maxd
 *   lengths[]      valid steps F_b of every item, 1 <= F_b <= T_gen - maxd
 *   speed[]        speed factor of every item, finite and > 0; NULL: no speed adjustment
 * delay[], lengths[] and speed[] are HOST arrays in both forms, as in the ragged calls.  Packed layouts as there: item b behind item b-1.
 * Every step is exact: the code kernels move integers; the speed kernel spells out the rounding of every binary32 operation, so each
 * output sample is one fixed bit pattern.  NC_EINVAL, before anything is launched, for: B <= 0; a null pointer (speed
 * excepted); C != n_codebooks or C > 32; a negative delay; T_gen <= maxd; a length <= 0 or > T_gen - maxd; a speed that is not finite or
 * <= 0; by the decode calls also min_valid < 0 or max_valid >= codebook_size (a code the mask lets through would index past the
 * codebook; Dia's 0 .. 1023 is DAC 44.1 kHz's whole codebook).  NC_ESTATE without weights.
 *
 * replaces: Dia.GenerateOutput                       Models/Dia.cs:1010-1093: BuildRevertIndices / RevertAudioDelay (Modules/Dia/
 *           AudioUtils.cs:108-176), the cut of the last maxd steps and the mask of codes outside [min_valid, max_valid] to 0 (Dia.cs:
 *           1039-1044; MinValidCodebookIndex = 0, MaxValidCodebookIndex = 1023, Dia.cs:53-58), Decode of item b at its own length
 *           (Dia.cs:1055-1058), AdjustSpeed (Dia.cs:947-966, below).  pcm_packed receives out_lens[b] samples per item.  Without speed,
 *           item b equals nc_dac_decode_code_matrix on its reverted [F_b, C] codes alone, bit for bit.
 * nc_dia_output_query (host arithmetic: nothing is launched): frames_out[b] = F_b, decoded_lens[b] = the decoded samples L_b,
 *           out_lens[b] = nc_dia_adjust_speed_len(L_b, speed[b]) (L_b without speed); outputs nullable. */
NC_API nc_status nc_dia_output_query(const nc_codec* h, int32_t B, int64_t T_gen, int32_t C, const int32_t* delay, const int64_t* lengths,
                                     const float* speed, int64_t* frames_out, int64_t* decoded_lens, int64_t* out_lens);
NC_API nc_status nc_dia_decode_output(nc_codec* h, const int64_t* codes_delayed, int32_t B, int64_t T_gen, int32_t C, const int32_t* delay,
                                      const int64_t* lengths, int64_t min_valid, int64_t max_valid, const float* speed, float* pcm_packed);
NC_API nc_status nc_dia_decode_output_dev(nc_codec* h, const int64_t* codes_delayed, int32_t B, int64_t T_gen, int32_t C, const int32_t* delay,
                                          const int64_t* lengths, int64_t min_valid, int64_t max_valid, const float* speed,
                                          float* pcm_packed);
/* The pieces on their own: device pointers, asynchronous on `hip_stream` (NULL = null stream), no handle.
 * replaces: AudioUtils.BuildDelayIndices / ApplyAudioDelay   Modules/Dia/AudioUtils.cs:19-94 (the voice prompt, Dia.cs:387-393):
 *           out[b, t, c] = t - delay[c] < 0 ? bos : codes[b, t - delay[c], c], int64 [B, T, C].  `pad` is taken as ApplyAudioDelay takes
 *           it and never written: its mask `t - delay[c] >= T` cannot fire for delay >= 0.
 * replaces: AudioUtils.BuildRevertIndices / RevertAudioDelay Modules/Dia/AudioUtils.cs:108-176 with the cut and the mask of Dia.cs:1039-1044:
 *           out[b, t, c] = codes[b, min(t + delay[c], T - 1), c] for t < T - maxd, values outside [min_valid, max_valid] written as 0;
 *           out int64 [B, T - maxd, C].  RevertAudioDelay's pad mask tests the index AFTER the clamp to T - 1 and cannot fire: no pad argument. */
NC_API nc_status nc_dia_apply_delay_dev(int device_index, const int64_t* codes, int32_t B, int64_t T, int32_t C, const int32_t* delay, int64_t pad,
                                        int64_t bos, int64_t* out, void* hip_stream);
NC_API nc_status nc_dia_revert_delay_dev(int device_index, const int64_t* codes, int32_t B, int64_t T, int32_t C, const int32_t* delay,
                                         int64_t min_valid, int64_t max_valid, int64_t* out, void* hip_stream);
/* The same values in the packed layout nc_dac_decode_codes_ragged reads (the first launch of nc_dia_decode_output on its own): item b as
 * [C, lengths[b]] row-major, item after item, 1 <= lengths[b] <= T - maxd (a HOST array). */
NC_API nc_status nc_dia_revert_pack_dev(int device_index, const int64_t* codes, int32_t B, int64_t T, int32_t C, const int32_t* delay,
                                        const int64_t* lengths, int64_t min_valid, int64_t max_valid, int64_t* out_packed, void* hip_stream);
/* replaces: Dia.AdjustSpeed                          Models/Dia.cs:947-966 through TorchUtils.Interp (Utils/TorchUtils.cs:58-82) on rows of
 *           packed PCM: row b of lens[b] samples -> nc_dia_adjust_speed_len(lens[b], speed[b]) samples, y = offset * x + slope at
 *           x = linspace(0, L - 1, T)[i] (binary32: step = (L - 1) / (T - 1); i < T / 2: i * step, else (L - 1) - (T - 1 - i) * step,
 *           each position one fused multiply-add as ATen's CPU kernel evaluates it; offset * x and + slope are rounded separately).
 *           A row whose length does not change is copied.  out_packed must not overlap pcm_packed.
 * nc_dia_adjust_speed_len: `(int)(L / speed)` in binary32 with AdjustSpeed's early returns -- L where |speed - 1| < 1e-5, where the
 *           quotient truncates to 0 or to L; -1 for L <= 0, a speed that is not finite or <= 0, or a quotient of 2^31 or more. */
NC_API int64_t nc_dia_adjust_speed_len(int64_t L, float speed);
NC_API nc_status nc_dia_adjust_speed_dev(int device_index, const float* pcm_packed, int32_t B, const int64_t* lens, const float* speed,
                                         float* out_packed, void* hip_stream);

/* -------------------------------------------------------------------------------------- Dia prompt stage
 * What Dia runs between its voice prompts and the language model's delayed prefill, as device kernels (csrc/nc_dia.hip): the
 * prompts of a batch are mixed to mono, encoded as ONE ragged batch and written as the delayed prefill without leaving HBM.
 *   pcm_packed   prompt b behind prompt b-1: lengths[b] frames of channels[b] interleaved samples ([n][ch]; channels NULL: all mono)
 *   lengths[]    samples per channel of every prompt; 0: no prompt (a null entry of the reference's list, or an item past its end)
 *   delay[]      C non-negative steps (DataConfig.DelayPattern), maxd = max(delay); C = the model's n_codebooks, at most 32
 *   prefill_out  int32 [B, T_max, C], Dia's layout (C fastest), T_max = max_b F_b + maxd with F_b the model's frames of prompt b (the
 *                length rule of nc_dac_ragged_query; 0 without a prompt).  With s = t - delay[c]:
 *                  prefill[b, t, c] = bos for s <= 0, codes_b[c][s - 1] for 1 <= s <= F_b, -1 behind it
 *                -1 is the torch.full value of Dia.cs:354-358, not `pad`.  `pad` is taken as ApplyAudioDelay takes it and never written:
 *                its mask `t - delay[c] >= T` cannot fire for delay >= 0.
 *   steps_out    int32 [B], a HOST array in both forms (nullable): the prefill steps F_b + 1, 1 without a prompt
 * lengths[], channels[] and delay[] are HOST arrays in both forms, as in the ragged calls.  Every value is a fixed bit pattern: the mix
 * spells out the rounding of its binary32 sum and division, the encode is nc_dac_encode_ragged_dev unchanged (prompt b's codes are those of
 * nc_dac_encode on it alone, bit for bit), the prefill moves integers.
 * NO RESAMPLING.  Dia.LoadAudio calls ResampleLinear where the file's rate differs from the model's and DISCARDS the result (Dia.cs:870-874):
 * the prompt is encoded at its own rate as if it were the model's.  These calls do the same and take no rate; a caller who wants the
 * obvious intent runs nc_audio_resample_linear_dev on the prompt first.
 * NC_EINVAL, before anything is launched (the handle stays usable): B <= 0; a null pointer (channels and steps_out excepted; pcm_packed may
 * be NULL when every length is 0); C != n_codebooks or C outside [1, 32]; a negative delay; a negative length or one above 2^30;
 * channels[b] <= 0; T_max == 0 (no prompt and no delay: nothing holds the BOS row); bos or pad outside int32; a grid that does not fit.
 * NC_ESTATE without weights.
 *
 * replaces: Dia.LoadAudio's mono mix                 Models/Dia.cs:851-864 (one launch per 32 prompts, only where a prompt has channels > 1),
 *           Dia.Encode of every prompt at its own length  Models/Dia.cs:988-1001 (the ragged encode over the prompts with F_b > 0, all C
 *           codebooks; with no prompt at all nothing is encoded),
 *           Dia.PrepareAudioPrompt                   Models/Dia.cs:329-400 with BuildDelayIndices / ApplyAudioDelay (Modules/Dia/
 *           AudioUtils.cs:19-94): one launch per 32 items writes every step of the prefill, the -1 fill included.
 *           B is PrepareAudioPrompt's `batch` = max(batchSize, prompts.Count) (Dia.cs:348).  With maxd == 0 the reference throws on its
 *           own copy (rows 1..F_b of a tensor of max F_b rows); here the closed form holds and the longest prompt's last frame is cut.
 * nc_dia_prompt_query (host arithmetic: nothing is launched): frames_out[b] = F_b, steps_out[b] = F_b + 1, *T_max_out; outputs nullable. */
NC_API nc_status nc_dia_prompt_query(const nc_codec* h, int32_t B, int32_t C, const int32_t* delay, const int64_t* lengths, int64_t* frames_out,
                                     int32_t* steps_out, int64_t* T_max_out);
NC_API nc_status nc_dia_encode_prompts(nc_codec* h, const float* pcm_packed, int32_t B, const int64_t* lengths, const int32_t* channels, int32_t C,
                                       const int32_t* delay, int64_t bos, int64_t pad, int32_t* prefill_out, int32_t* steps_out);
NC_API nc_status nc_dia_encode_prompts_dev(nc_codec* h, const float* pcm_packed, int32_t B, const int64_t* lengths, const int32_t* channels,
                                           int32_t C, const int32_t* delay, int64_t bos, int64_t pad, int32_t* prefill_out, int32_t* steps_out);
/* The pieces on their own: device pointers, asynchronous on `hip_stream` (NULL = null stream), no handle.
 * replaces: Dia.PrepareAudioPrompt on codes that exist already: codes_packed as nc_dac_encode_ragged writes them (item b as [C, frames[b]]
 *           row-major, int64, item after item; frames[] a HOST array, 0: no prompt; NULL allowed when every frames[b] is 0) -> out int32
 *           [B, T_max, C] by the closed form above.  Any 1 <= C <= 32; T_max >= max(frames) + maxd and > 0: steps past a prompt follow the
 *           closed form (-1, or bos up to delay[c]).  Codes are narrowed as `prompt.to(torch.int32)` narrows them (the low 32 bits). */
NC_API nc_status nc_dia_prefill_pack_dev(int device_index, const int64_t* codes_packed, int32_t B, const int64_t* frames, int32_t C,
                                         const int32_t* delay, int64_t bos, int64_t pad, int64_t T_max, int32_t* out, void* hip_stream);
/* replaces: Dia.LoadAudio's mono mix                 Models/Dia.cs:851-864 over a packed ragged batch: prompt b is n_frames[b] frames of
 *           channels[b] interleaved samples -> n_frames[b] samples, prompt after prompt (HOST arrays; n_frames[b] >= 0, channels[b] >= 1).
 *           A binary32 running sum in channel order, one division by (float)channels, as nc_audio_mix_to_mono_dev; a prompt of one channel
 *           is copied bit for bit.  out_packed must not overlap in_packed. */
NC_API nc_status nc_audio_mix_to_mono_ragged_dev(int device_index, const float* in_packed, int32_t B, const int64_t* n_frames,
                                                 const int32_t* channels, float* out_packed, void* hip_stream);

/* ------------------------------------------------------------------------------------ Dia sampling stage
 * What Dia runs once per generated frame between its language model's logits and the next row of the delayed code matrix, as ONE launch
 * (csrc/nc_dia.hip).  With the two stages above: prompt -> [caller's LM] -> next code row -> PCM, no host work in between.
 *   logits     float32 [2B, C, V], row 2b unconditional, row 2b + 1 conditional (the view of Dia.cs:531-535); 1 <= C <= 32, V <= 4096.
 *              fp32 ONLY: a caller with bf16 logits converts first.  The reference converts before sampling too (Dia.cs:553) but runs
 *              the guidance and the masks in the compute dtype; that arithmetic is NOT reproduced, the guidance here is binary32.
 *   uniform    float32 [B, C] in [0, 1): the draw of every row, SUPPLIED by the caller (deviation 1: the reference's multinomial on
 *              torch's generator is not reproducible; a supplied uniform is).  Required, also when temperature selects the greedy path.
 *   tokens     int64 [B, C];  bad int32 [B]
 * Per row (b, c), every value one fixed bit pattern (fl = one binary32 rounding; the unit is built with -ffp-contract=off):
 *   1 guidance   g = cond + fl(cfg_scale * fl(cond - uncond))                                                        Dia.cs:538
 *   2 masks      v > eos: -inf;  c >= 1 and v >= eos: -inf;  on channel 0 g[eos] = fl(g[eos] * 0.8f)                 Dia.cs:541-548
 *   3 greedy     temperature < 1e-5f: the token is argmax(g) in ATen's order (first maximum; a NaN beats every number, first NaN
 *                wins: nc_argmax_before, nc_math.h) and the row is done                                             Dia.cs:434-437
 *   4 EOS rule   if that argmax is not eos, g[eos] = -inf                                                            Dia.cs:439-448
 *   5            x = fl(g / temperature), a true IEEE division                                                       Dia.cs:451
 *   6 survivors  the top_k largest x > -inf, ordered by (value descending, index ascending); 1 <= top_k <= 64.  ATen leaves the order
 *                of topk / sort among equal values open: this order is the project's definition (deviation 2).  -inf is never a
 *                survivor (nc_expf clamps its argument at -87 and would not map it to 0)                              Dia.cs:454-466
 *   7 nucleus    only if top_p < 1: e_j = nc_expf(x_j - x_0); S = e_0 + e_1 + ... added in survivor order; p_j = fl(e_j / S) with
 *                the cumulative c_j added in the same order; survivor j >= 1 is removed when c_{j-1} > top_p         Dia.cs:468-494
 *   8 draw       S' = the kept e_j added in survivor order, q_j = fl(e_j / S') with the cumulative d_j; the token is the first kept j
 *                with u < d_j, the last kept one if rounding leaves none                                             Dia.cs:497-499
 *   9 bad rows   a NaN among the masked g of a sampled row, no survivor, or a survivor of +inf: token -1 and bad[b] != 0 (the reference
 *                throws inside multinomial there).  nc_dia_sample_* write bad[b] = 0 or 1; the step ORs into it (the caller zeroes it).
 * nc_dia_sample_params: cfg_scale, temperature, top_p finite, temperature >= 0, top_p > 0 (>= 1: no nucleus); eos in [0, V); pad is what
 * the step writes behind EOS.  Reference defaults (Dia.Generate, Dia.cs:615-624): 3.0, 1.2, 0.95, top_k 45; eos / pad 1024 / 1025.
 * NC_EINVAL, before anything is launched, for: a null pointer; B <= 0; C < 1 or C > 32; eos < 0 or eos >= V; V > 4096; top_k outside
 * [1, 64]; temperature, top_p or cfg_scale not finite; temperature < 0; top_p <= 0; by the step also a negative delay, step < 0 or
 * step >= L, max_tokens > L.
 *
 * replaces: Dia.DecoderStep from the logits on        Models/Dia.cs:530-560 with SampleNextToken (Dia.cs:424-501): nc_dia_sample_dev
 *           (device pointers, asynchronous on `hip_stream`, no handle) and nc_dia_sample_host -- the same arithmetic as plain serial
 *           C++ on HOST pointers, no device: for a CPU caller and for checking a device result (written independently of the kernel;
 *           the two share nc_math.h and nothing else, and agree bit for bit). */
typedef struct nc_dia_sample_params {
    float cfg_scale, temperature, top_p;
    int32_t top_k, eos, pad;
} nc_dia_sample_params;
NC_API nc_status nc_dia_sample_dev(int device_index, const float* logits, int32_t B, int32_t C, int32_t V, const nc_dia_sample_params* params,
                                   const float* uniform, int64_t* tokens, int32_t* bad, void* hip_stream);
NC_API nc_status nc_dia_sample_host(const float* logits, int32_t B, int32_t C, int32_t V, const nc_dia_sample_params* params, const float* uniform,
                                    int64_t* tokens, int32_t* bad);
/* replaces: the EOS countdown of Dia.Generate         Models/Dia.cs:706-746 and DecoderOutput.UpdateOne (Modules/Dia/DecoderOutput.cs:
 *           71-86) behind the sampling above, sampling + bookkeeping + write in ONE launch, no .item() round trip.
 *   state      DEVICE int64 [3, B]: detected (0 / 1), countdown (-1 idle, > 0 running, 0 done), finished (-1 none);
 *              nc_dia_generate_state_init_dev writes 0 / -1 / -1 (Dia.cs:667-669)
 *   generated  DEVICE int32 [B, L, C]: DecoderOutput.GeneratedTokens, the buffer nc_dia_encode_prompts prefilled (-1: not written)
 *   delay[]    HOST, C non-negative steps, D = max(delay);  step = the reference's currentStepIdx s;  M = max_tokens
 * Per item, with tok[] the sampled row:
 *   active = countdown != 0;  trigger = active && ((!detected && tok[0] == eos) || s >= M - D);  detected |= trigger
 *   trigger && countdown < 0:  countdown = D, finished = s
 *   countdown > 0:  a = D - countdown; tok[c] = eos where a == delay[c], pad where a > delay[c];  countdown -= 1
 *   generated[b, s, c] = (int32)tok[c] -- with apply_mask != 0 only where the slot still holds -1 (UpdateOne's mask; the caller
 *   computes !bosOver on the host from the prefill steps, Dia.cs:749-755).  Items whose countdown is 0 are still sampled and written, as
 *   in the reference.  active_out[b] (DEVICE int32 [B]) = countdown != 0 after the step: poll it whenever, no per-step synchronisation. */
NC_API nc_status nc_dia_generate_state_init_dev(int device_index, int32_t B, int64_t* state, void* hip_stream);
NC_API nc_status nc_dia_generate_step_dev(int device_index, const float* logits, int32_t B, int32_t C, int32_t V, const nc_dia_sample_params* params,
                                          const float* uniform, const int32_t* delay, int64_t step, int64_t max_tokens, int32_t apply_mask,
                                          int64_t* state, int32_t* generated, int64_t L, int32_t* active_out, int32_t* bad, void* hip_stream);
/* replaces: the lengths of Dia.Generate               Models/Dia.cs:775-782 (host arithmetic, no device): finished[] is a HOST copy of the
 *           third row of `state`; a finished of -1 becomes final_step - maxd; lengths_out[b] = max(0, finished - prefill_steps[b]);
 *           *T_gen_out = max(lengths_out) + maxd.  NC_EINVAL for a null pointer (T_gen_out excepted), B <= 0 or maxd < 0.
 * replaces: the copy into generatedCodes              Models/Dia.cs:786-801, one launch per 32 items: out int64 [B, T_gen, C], T_gen =
 *           max(lengths) + maxd, out[b, t, c] = generated[b, prefill_steps[b] + t, c] for t < lengths[b] + maxd, `pad` behind it --
 *           exactly the codes_delayed nc_dia_decode_output_dev takes, with these lengths.  prefill_steps[] and lengths[] are HOST arrays.
 *           NC_EINVAL for a null pointer, B <= 0, C outside [1, 32], maxd < 0, a negative entry, T_gen == 0 (nothing was generated) or
 *           prefill_steps[b] + lengths[b] + maxd > L. */
NC_API nc_status nc_dia_generate_lengths(int32_t B, const int64_t* finished, const int32_t* prefill_steps, int64_t final_step, int64_t maxd,
                                         int64_t* lengths_out, int64_t* T_gen_out);
NC_API nc_status nc_dia_generate_collect_dev(int device_index, const int32_t* generated, int32_t B, int64_t L, int32_t C,
                                             const int32_t* prefill_steps, const int64_t* lengths, int64_t maxd, int64_t pad, int64_t* out,
                                             void* hip_stream);

/* ------------------------------------------------------------------------------------ round-trip quality
 * How good a decode is, next to the audio it came from: L1, SI-SDR and the multi-scale mel distance of the DAC paper, with the STFT and the
 * mel spectrogram they stand on.  Every value is one fixed bit pattern (fl = one binary32 rounding; no libm on the data path; the units
 * are built with -ffp-contract=off), stated here so that the *_host twins (csrc/nc_quality_host.hip: plain serial C++ on HOST pointers,
 * no device, sharing nc_math.h and the table builders below with the kernels and nothing else) and the kernels agree bit for bit.
 *   basis   window W (a power of two, 32..2048), k = 0..W/2, n = 0..W-1, evaluated in binary64 and rounded once:
 *             C[k][n] = fl(w(n) cos(2 pi ((k n) mod W) / W)),  S[k][n] = fl(-w(n) sin(2 pi ((k n) mod W) / W))
 *           window NC_WINDOW_HANN: w(n) = 0.5 - 0.5 cos(2 pi n / W) (torch.hann_window, periodic);  NC_WINDOW_ONES: w = 1.
 *   STFT    center = true: reflect padding of W/2 each side (so n > W/2), hop H (1 <= H <= min(W, 512)), frames = 1 + n / H.
 *           re[k][t] = ONE chain over n ascending of fmaf(C[k][n], x_pad[t H + n], acc) from acc = 0; im the same with S;
 *           |X|[k][t] = sqrtf(fl(fl(re re) + fl(im im))).  Output layouts: complex64 [W/2+1][frames] (re, im interleaved).
 *   mel     fb[m][k] and the support [lo[m], hi[m]) from nc_audio_mel_filterbank (n_fft = W);  mel[m][t] = ONE chain over k = lo..hi-1
 *           ascending of fmaf(fb[m][k], |X|[k][t], acc) from 0; a band with empty support is 0.  Output float [n_mels][frames].
 *   rows    a row is one channel of one clip (SISDRLoss.PrepareInputs); x = estimate, y = reference, n = compared samples.
 *           Sums are binary64, serial: samples ascending within blocks of 128, then the blocks ascending.
 *             n_bad  = the non-finite samples of x plus those of y;  l1 = fl(sum |fl(x - y)| / n)
 *             xc = x - sum(x)/n, yc = y - sum(y)/n in binary64;  EPS = (double)1e-8f
 *             scale = (sum(xc yc) + EPS) / (sum(yc yc) + EPS);  target = scale scale sum(yc yc);  error = sum((xc - scale yc)^2)
 *             si_sdr_db = fl(10.0f * nc_log10f(fl(min(target / (error + EPS) + EPS, FLT_MAX))))      (the negative of SISDRLoss.forward)
 *           per scale i, over the n_mels x frames mel values X (of x) and Y (of y): per frame the bands ascending, then the frames
 *           ascending, in binary64:
 *             mel_mag[i] = fl(sum |fl(X - Y)| / count);  mel_log[i] = fl(sum |fl(L(X) - L(Y))| / count),  L(v) = nc_log10f(fl(c c)),
 *             c = max(v, clamp_eps)   (MelSpectrogramLoss.forward with pow = 2)
 *             mel_distance = fl(sum_i (log_weight mean_log_i + mag_weight mean_mag_i)) on the binary64 means, i ascending
 *           A row with n_bad != 0 has NaN in l1, si_sdr_db, mel_distance and the n_scales used mel entries; other rows are untouched.
 * nc_quality_cfg: 1 <= n_scales <= 8; W[i] as above; H[i] = 0 means W[i] / 4; 1 <= n_mels[i] <= 512; fmax[i] = 0 means sample_rate / 2;
 * clamp_eps >= 1e-18f (its square must be a normal binary32).  Reference defaults: clamp_eps 1e-5f, both weights 1.
 * off[] / n[] / out_off[] / ref_off[] / est_off[] are HOST arrays of ELEMENT offsets and lengths into the packed buffers: the packed input
 * of a ragged encode and the packed output of the ragged decode are compared in place.
 * NC_EINVAL, before anything is launched: a null pointer; B < 1 or B > 32767; n[b] <= W/2 for a requested window; a negative offset; W not
 * a power of two in 32..2048; H outside [1, min(W, 512)]; n_mels outside [1, 512]; sample_rate <= 0; fmin < 0; fmax <= fmin; an unknown
 * window; n_scales outside [1, 8]; clamp_eps < 1e-18f or a weight that is not finite.
 *
 * replaces: DSP.STFT                                 AudioTools/AudioTensorDSP.cs:716-809 (nc_audio_stft_dev / _host; frames: the last
 *           dimension of its result, -1 where n <= W/2)
 * replaces: DSP.MelFilterbank                        AudioTools/AudioTensorDSP.cs:844-894 with HertzToMel / MelToHertz
 *           (Utils/AudioExtensions.cs:31-44), in binary64, rounded once; fb [n_mels][n_fft/2+1], lo / hi [n_mels] (nullable).  The
 *           reference builds it for max(W, 2048) (FFTLengths, :920), which its matmul cannot take for W < 2048; here n_fft = W.
 * replaces: DSP.MelSpectrogram                       AudioTools/AudioTensorDSP.cs:595-669 (hann window)
 * replaces: L1Loss / SISDRLoss / MelSpectrogramLoss  Modules/DAC/L1Loss.cs, SISDRLoss.cs:100-164, MelSpectrogramLoss.cs:116-137 as
 *           per-row evaluation metrics: nc_quality_metrics_dev (DEVICE buffers and DEVICE out[B], asynchronous on `hip_stream`),
 *           nc_quality_metrics (HOST buffers, synchronous) and nc_quality_metrics_host (no device). */
#define NC_WINDOW_HANN 0
#define NC_WINDOW_ONES 1
#define NC_QUALITY_MAX_SCALES 8
typedef struct nc_quality_cfg {
    int32_t n_scales;
    int32_t W[8], H[8], n_mels[8];   /* [NC_QUALITY_MAX_SCALES] each */
    float fmin[8], fmax[8];
    float clamp_eps, log_weight, mag_weight;
} nc_quality_cfg;
typedef struct nc_quality_row {
    float l1, si_sdr_db, mel_distance;
    float mel_log[8], mel_mag[8];    /* [NC_QUALITY_MAX_SCALES] each */
    int32_t n_bad;
} nc_quality_row;
NC_API int64_t nc_audio_stft_frames(int64_t n, int32_t W, int32_t H);
NC_API nc_status nc_audio_dft_basis(int32_t W, int32_t window, float* C /* [W/2+1][W] */, float* S);
NC_API nc_status nc_audio_mel_filterbank(int32_t sample_rate, int32_t n_mels, int32_t n_fft, float fmin, float fmax, float* fb, int32_t* lo,
                                         int32_t* hi);
NC_API nc_status nc_audio_stft_dev(int device_index, const float* pcm, int32_t B, const int64_t* off, const int64_t* n, int32_t W, int32_t H,
                                   int32_t window, float* out_c64, const int64_t* out_off, void* hip_stream);
NC_API nc_status nc_audio_stft_host(const float* pcm, int32_t B, const int64_t* off, const int64_t* n, int32_t W, int32_t H, int32_t window,
                                    float* out_c64, const int64_t* out_off);
NC_API nc_status nc_audio_mel_spectrogram_dev(int device_index, const float* pcm, int32_t B, const int64_t* off, const int64_t* n,
                                              int32_t sample_rate, int32_t W, int32_t H, int32_t n_mels, float fmin, float fmax, float* out,
                                              const int64_t* out_off, void* hip_stream);
NC_API nc_status nc_audio_mel_spectrogram_host(const float* pcm, int32_t B, const int64_t* off, const int64_t* n, int32_t sample_rate, int32_t W,
                                               int32_t H, int32_t n_mels, float fmin, float fmax, float* out, const int64_t* out_off);
NC_API nc_status nc_quality_metrics_dev(int device_index, const float* ref, const int64_t* ref_off, const float* est, const int64_t* est_off,
                                        const int64_t* n, int32_t B, int32_t sample_rate, const nc_quality_cfg* cfg, nc_quality_row* out,
                                        void* hip_stream);
NC_API nc_status nc_quality_metrics(int device_index, const float* ref, const int64_t* ref_off, const float* est, const int64_t* est_off,
                                    const int64_t* n, int32_t B, int32_t sample_rate, const nc_quality_cfg* cfg, nc_quality_row* out);
NC_API nc_status nc_quality_metrics_host(const float* ref, const int64_t* ref_off, const float* est, const int64_t* est_off, const int64_t* n,
                                         int32_t B, int32_t sample_rate, const nc_quality_cfg* cfg, nc_quality_row* out);

/* ------------------------------------------------------------------------------------ loudness
 * ITU-R BS.1770 K-weighting, gated integrated loudness (LUFS), normalisation to a target level and the gain that restores a stored
 * level.  Every value is one fixed bit pattern (fl = one binary32 rounding; binary64 operations are single IEEE operations, never fused;
 * no libm on the data path; the units are built with -ffp-contract=off), stated here so that the *_host twins (csrc/nc_loudness_host.hip:
 * plain serial C++ on HOST pointers, no device, sharing nc_math.h, the table builder and the argument checks with the kernels and
 * nothing else) and the kernels (csrc/nc_loudness.hip) agree bit for bit.
 *   clips   a clip has C channels, 1 <= C <= 5, with weights G = {1, 1, 1, 1.41f, 1.41f} (LoudnessMeter.cs:36), one length n[b] and C
 *           ELEMENT offsets off[b C + c] into a packed float buffer: any planar layout, the packed buffers of the ragged calls in place.
 *           off[] / n[] / out_off[] / db[] are HOST arrays.  B C <= 32767 (nc_audio_kweight: R rows <= 32767).
 *   coeffs  nc_loudness_cfg.filter = NC_KWEIGHT_REFERENCE: the binary32 literals of LoudnessMeter.cs:41-52, widened, at ANY sample rate (as
 *           the reference does);  NC_KWEIGHT_DESIGNED: per rate, in binary64, the analog prototypes of the BS.1770 constants through the
 *           bilinear transform, K = tan(pi f0 / rate), every stage normalised by a0 = 1 + K/Q + K^2:
 *             high shelf  f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196, Vh = 10^(G/20), Vb = Vh^0.4996667741545416:
 *                         b = (Vh + Vb K/Q + K^2, 2 (K^2 - Vh), Vh - Vb K/Q + K^2) / a0,  a = (1, 2 (K^2 - 1) / a0, (1 - K/Q + K^2) / a0)
 *             high pass   f0 = 38.13547087602444, Q = 0.5003270373238773: b = (1, -2, 1) (not normalised, as in the recommendation), a as above
 *           At 48 kHz this gives the constants back (to 1e-15 of their decimal form, 6e-8 of the binary32 literals).  A round-number design
 *           (RBJ shelf +4 dB / 1500 Hz / Q 1/sqrt(2), RBJ high pass 38 Hz / Q 0.5) does not: it misses them by 1.1e-4 and, in the high
 *           pass's normalised numerator, by 1e-2.
 *           nc_audio_kweight_coeffs exports b[2][3], a[2][3] (stage 0 = shelf, 1 = high pass; a[s][0] = 1).
 *   filter  the cascade shelf -> high pass, each biquad in transposed direct form II, zero initial state, as a 4-state system
 *           s' = A s + B x, y = C s + D x (s0, s1: the shelf's registers; s2, s3: the high pass's), A, B, C, D in binary64.
 *   tables  block length L = 64; in binary64, powers by repeated left multiplication (A^(k+1) B = A (A^k B), C A^(r+1) = (C A^r) A,
 *           A^(k+1) = A A^k), every dot product summed in ascending index from the first product:
 *             h[0] = D, h[k] = C (A^(k-1) B);  Hm[r][j] = fl(h[r - j]) for j <= r, else 0;  Cm[i][j] = fl((A^(L-1-j) B)[i]);
 *             Gs[r] = C A^r (1 x 4) and M = A^L (4 x 4) stay binary64.        (nc_audio_kweight_tables)
 *   block q of a row, x = 0 past the row end, s_0 = 0:
 *             u[r] = ONE chain over j = 0..63 ascending of fmaf(Hm[r][j], x[64 q + j], acc) from acc = 0;  v[i] the same with Cm[i]
 *             y[64 q + r] = fl((double)u[r] + g),  g = ((Gs[r][0] s_q[0] + Gs[r][1] s_q[1]) + Gs[r][2] s_q[2]) + Gs[r][3] s_q[3]
 *             s_{q+1}[i] = m + (double)v[i],       m = ((M[i][0] s_q[0] + M[i][1] s_q[1]) + M[i][2] s_q[2]) + M[i][3] s_q[3]
 *   energy  N = (int)(0.4f rate), S = (int)((0.4f rate) 0.25f) in binary32 (LoudnessMeter.cs:140-141); J = (n - N) / S + 1 blocks for
 *           n >= N, else 0.  Cell i = samples [i S, (i + 1) S): the binary64 sum of fl(y y), samples ascending within sub-blocks of 128
 *           counted from the cell's start, then the sub-blocks ascending.  Block j = ((cell j + cell j+1) + cell j+2) + cell j+3, then
 *           the N - 4 S samples [(j + 4) S, j S + N) added one by one;  z[c][j] = sum / (double)N;  W_j = sum_c (double)G_c z[c][j],
 *           c ascending.
 *   gates   on the binary64 sums.  Absolute: block j passes iff W_j > Ka = 0x1.f791ec6e1d5aap-24 (the binary64 nearest 10^-6.9309, i.e.
 *           -0.691 + 10 log10 W > -70).  za[c] = (sum of z[c][j] over the passing j, ascending) / max(count, 1);  Wa = sum_c G_c za[c].
 *           Relative: block j passes iff it passes the absolute gate and W_j > 0.1 Wa;  zr[c] and Wr likewise.
 *   result  lufs = max(fl(-0.691f + fl(10.0f nc_log10f(fl(Wr)))), -70.0f); -70.0f where fl(Wr) is below the smallest normal (an
 *           all-silent clip, a clip shorter than one block).  gain = nc_expf(fl(fl(target_db - lufs) GAIN_FACTOR)),
 *           GAIN_FACTOR = 0.11512925464970229f.  n_bad = the non-finite samples of the clip (all channels, clamped to INT32_MAX); a clip
 *           with n_bad != 0 has NaN in lufs and gain and 0 in both pass counts; other clips are untouched.
 *   gain    nc_loudness_normalize writes fl(x gain) per sample (the quiet NaN 0x7fc00000 where gain is NaN) to out_off, which may equal
 *           off (in place), and returns the rows so that the measured level can be stored;  nc_audio_apply_gain_db writes
 *           fl(x nc_expf(fl(db[b] GAIN_FACTOR))): with db = stored lufs - target_db it undoes a normalisation after a decode.
 * Deviations from the reference: the exact recursion instead of its two filter paths (ApplyFilterCPU's LFilter indexes the first
 * dimension of a 3-D tensor; ApplyFilterGPU truncates the high pass, pole radius 0.995, at 512 taps and returns n + 1 samples);
 * division by the integer N instead of multiplication by 1.0f / (0.4f rate); gate comparisons on the binary64 sums instead of binary32
 * log10 values.  AudioSignal.Loudness() zero-pads a clip shorter than 0.5 s; here a clip shorter than one block reports -70.
 * NC_EINVAL, before anything is launched: a null pointer; B < 1, C outside [1, 5], B C > 32767; a negative offset or length;
 * sample_rate < 10 (N or S would be 0); an unknown filter; a target or a db[b] that is not finite.
 *
 * replaces: LoudnessMeter.IntegratedLoudness / NormalizeAudio   AudioTools/LoudnessMeter.cs:127-207
 * replaces: AudioSignal.Loudness / Normalize                    AudioTools/AudioSignal.cs:847-940
 *           each as _dev (DEVICE buffers, asynchronous on `hip_stream`), plain (HOST buffers, synchronous) and _host (no device). */
#define NC_KWEIGHT_REFERENCE 0
#define NC_KWEIGHT_DESIGNED 1
#define NC_LOUDNESS_MAX_CHANNELS 5
typedef struct nc_loudness_cfg {
    int32_t filter;      /* NC_KWEIGHT_* */
    float target_db;     /* the level `gain` leads to; the reference's default is -24 */
} nc_loudness_cfg;
typedef struct nc_loudness_row {
    float lufs, gain;
    int32_t n_blocks, n_pass_abs, n_pass_rel, n_bad;
} nc_loudness_row;
NC_API nc_status nc_audio_kweight_coeffs(int32_t sample_rate, int32_t filter, double* b /* [2][3] */, double* a /* [2][3] */);
NC_API nc_status nc_audio_kweight_tables(int32_t sample_rate, int32_t filter, float* Hm /* [64][64] */, float* Cm /* [4][64] */,
                                         double* Gs /* [64][4] */, double* M /* [4][4] */);
NC_API nc_status nc_audio_kweight_dev(int device_index, const float* pcm, int32_t R, const int64_t* off, const int64_t* n, int32_t sample_rate,
                                      int32_t filter, float* out, const int64_t* out_off, void* hip_stream);
NC_API nc_status nc_audio_kweight(int device_index, const float* pcm, int32_t R, const int64_t* off, const int64_t* n, int32_t sample_rate,
                                  int32_t filter, float* out, const int64_t* out_off);
NC_API nc_status nc_audio_kweight_host(const float* pcm, int32_t R, const int64_t* off, const int64_t* n, int32_t sample_rate, int32_t filter,
                                       float* out, const int64_t* out_off);
NC_API nc_status nc_loudness_dev(int device_index, const float* pcm, int32_t B, int32_t C, const int64_t* off, const int64_t* n,
                                 int32_t sample_rate, const nc_loudness_cfg* cfg, nc_loudness_row* out, void* hip_stream);
NC_API nc_status nc_loudness(int device_index, const float* pcm, int32_t B, int32_t C, const int64_t* off, const int64_t* n, int32_t sample_rate,
                             const nc_loudness_cfg* cfg, nc_loudness_row* out);
NC_API nc_status nc_loudness_host(const float* pcm, int32_t B, int32_t C, const int64_t* off, const int64_t* n, int32_t sample_rate,
                                  const nc_loudness_cfg* cfg, nc_loudness_row* out);
NC_API nc_status nc_loudness_normalize_dev(int device_index, const float* pcm, int32_t B, int32_t C, const int64_t* off, const int64_t* n,
                                           int32_t sample_rate, const nc_loudness_cfg* cfg, float* out, const int64_t* out_off,
                                           nc_loudness_row* rows, void* hip_stream);
NC_API nc_status nc_loudness_normalize(int device_index, const float* pcm, int32_t B, int32_t C, const int64_t* off, const int64_t* n,
                                       int32_t sample_rate, const nc_loudness_cfg* cfg, float* out, const int64_t* out_off,
                                       nc_loudness_row* rows);
NC_API nc_status nc_loudness_normalize_host(const float* pcm, int32_t B, int32_t C, const int64_t* off, const int64_t* n, int32_t sample_rate,
                                            const nc_loudness_cfg* cfg, float* out, const int64_t* out_off, nc_loudness_row* rows);
NC_API nc_status nc_audio_apply_gain_db_dev(int device_index, const float* pcm, int32_t B, int32_t C, const int64_t* off, const int64_t* n,
                                            const float* db, float* out, const int64_t* out_off, void* hip_stream);
NC_API nc_status nc_audio_apply_gain_db(int device_index, const float* pcm, int32_t B, int32_t C, const int64_t* off, const int64_t* n,
                                        const float* db, float* out, const int64_t* out_off);
NC_API nc_status nc_audio_apply_gain_db_host(const float* pcm, int32_t B, int32_t C, const int64_t* off, const int64_t* n, const float* db,
                                             float* out, const int64_t* out_off);

/* ------------------------------------------------------------------------------------ band-limited resampling
 * Windowed-sinc polyphase resampling of R rows (a row is one channel of one clip) from `src` to `dst` Hz: the resampler of the upstream
 * DAC pipeline (julius resample_frac, the family of torchaudio's resample), as one fixed bit pattern.  The host twin
 * (csrc/nc_resample_host.hip: plain serial C++ on HOST pointers, no device) and the kernels (csrc/nc_resample.hip) share the checks, the
 * geometry and the table builder (csrc/nc_resample.h) and nothing of the per-sample arithmetic; they agree bit for bit.
 *   ratio   g = gcd(src, dst), U = dst / g, D = src / g.  src == dst: every row is copied.
 *   config  nc_resample_cfg { zeros, rolloff }; a NULL pointer, zeros == 0 or rolloff == 0 stand for julius' defaults zeros = 24 and
 *           rolloff = the binary64 0.945, as julius holds it (widened from 0.945f, 24 * 441 / (160 rolloff) of 44100 -> 16000 lands a hair
 *           above 70 and W would be 71 where julius has 70).  A rolloff that is given is widened from binary32.  Admitted: 1 <= zeros <= 64,
 *           0.5 <= rolloff <= 1.
 *   geom    in binary64: base = min(U, D) rolloff;  W = ceil(zeros D / base) (the product first, then the
 *           quotient);  K = 2 W + D;  K4 = K rounded up to a multiple of 4.                              (nc_audio_resample_sinc_geom)
 *   table   h[U][K4] in binary64, rounded ONCE to binary32.  For k < K, with pi = 0x1.921fb54442d18p+1:
 *             t = ((-(double)i) / U + (double)(k - W) / D) base, clamped to [-zeros, zeros];  a = pi t;
 *             v = (a == 0 ? 1 : sin(a) / a) c c,  c = cos(a / (2 zeros));
 *           row i is divided by its own sum (k ascending from 0.0), so every phase has unity DC gain; for K <= k < K4 the tap is +0.
 *           sin and cos are libm's: the builder runs on the host only, the kernels and the twin of one process read the same table, and
 *           nothing on the data path depends on libm.  Two libm builds may differ in the last binary64 place, which moves a binary32
 *           rounding only next to a tie: tests hold the table within 1 ulp of binary32 of a binary64 restatement, not bit for bit.
 *                                                                                                        (nc_audio_resample_sinc_table)
 *   pad     xpad[j] = x[clamp(j - W, 0, n - 1)]: the edge sample repeated, as julius does; no padded copy is ever stored.
 *   chain   y[m U + i] = acc after acc = 0.0f; acc = fmaf(h[i][k], xpad[m D + k], acc) for k = 0 .. K4 - 1 ascending, in binary32.  The
 *           zero taps K .. K4 - 1 are part of the chain (they can turn -0 into +0 and meet a non-finite sample).
 *           A result that is a NaN is stored as the quiet NaN 0x7fc00000: the sign and payload of the NaN an invalid operation makes
 *           (0 x inf, inf - inf) differ between hosts and gfx950.
 *   length  n_out = ceil(n U / D), exact in int64 (nc_audio_resample_sinc_len; -1 on bad arguments).  Row r writes out[out_off[r] + j] for
 *           j < n_out only; a row of length 0 writes nothing.
 * off[] / n[] / out_off[] are HOST arrays of ELEMENT offsets and lengths, as in the loudness calls.
 * NC_EINVAL, before anything is launched: a null pointer; a rate < 1; R outside [1, 32767]; a negative offset; n[r] outside [0, 2^30]; a
 * config outside the admitted ranges; a table U K4 4 B above 4 MiB (the L2 of one XCD: 32000 -> 44100 passes with 641 KB, 44100 -> 44101
 * is refused); an output row [out + out_off[r], + n_out) that overlaps an input row [pcm + off[r'], + n[r']) (the lengths differ, so the
 * call never runs in place); a row whose n_out is above 2^31 - 256 (one launch).
 * Deviation from the reference: AudioSignal.ResampleFrac is not mirrored, because it does not do what its name says -- each of its two
 * stages adds 128 samples it never trims (4800 samples at 48 kHz become 4412 at 44.1 kHz, 2464 at 24 kHz); the filter is normalised to
 * sum 1 AFTER zero-stuffing, which cancels its own gain U (24 kHz -> 48 kHz halves the amplitude); and the half-width is 64 taps in the
 * UPSAMPLED domain, so for 48 kHz -> 44.1 kHz (U = 147) the 129 taps see at most one non-zero sample (a 0.5 sine comes out at 0.0055).
 * tests/test_resample_cpu.py restates it and asserts the three findings.
 *
 * replaces: AudioSignal.ResampleFrac                            AudioTools/AudioSignal.cs:962-1032
 *           as _dev (DEVICE buffers, asynchronous on `hip_stream`), plain (HOST buffers: upload, run, download) and _host (no device). */
typedef struct nc_resample_cfg {
    int32_t zeros;       /* zero crossings of the sinc on either side; 0 = 24 */
    float rolloff;       /* cutoff as a fraction of the lower Nyquist; 0 = 0.945 */
} nc_resample_cfg;
NC_API int64_t nc_audio_resample_sinc_len(int64_t n_in, int32_t src, int32_t dst);
NC_API nc_status nc_audio_resample_sinc_geom(int32_t src, int32_t dst, const nc_resample_cfg* cfg, int32_t* U, int32_t* D, int32_t* W, int32_t* K,
                                             int32_t* K4);
NC_API nc_status nc_audio_resample_sinc_table(int32_t src, int32_t dst, const nc_resample_cfg* cfg, float* h /* [U][K4] */);
NC_API nc_status nc_audio_resample_sinc_dev(int device_index, const float* pcm, int32_t R, const int64_t* off, const int64_t* n, int32_t src,
                                            int32_t dst, const nc_resample_cfg* cfg, float* out, const int64_t* out_off, void* hip_stream);
NC_API nc_status nc_audio_resample_sinc(int device_index, const float* pcm, int32_t R, const int64_t* off, const int64_t* n, int32_t src,
                                        int32_t dst, const nc_resample_cfg* cfg, float* out, const int64_t* out_off);
NC_API nc_status nc_audio_resample_sinc_host(const float* pcm, int32_t R, const int64_t* off, const int64_t* n, int32_t src, int32_t dst,
                                             const nc_resample_cfg* cfg, float* out, const int64_t* out_off);

/* ------------------------------------------------------------------------------------ inverse STFT, spectral masks, MFCC
 * From a spectrogram back to PCM, rectangles of a spectrogram set to a value, and cepstral coefficients -- on the packed buffers of the
 * forward transform above, so that a caller who removes a hum band or blanks a click never leaves them.  Every value is one fixed bit
 * pattern (fl = one binary32 rounding; no libm on the data path; -ffp-contract=off), stated here so that the *_host twins
 * (csrc/nc_spectral_host.hip: plain serial C++ on HOST pointers, no device) and the kernels (csrc/nc_spectral.hip) agree bit for bit; they
 * share nc_math.h, the checks and the table builders (csrc/nc_spectral.h) and nothing of the arithmetic on bins or samples.
 *   ISTFT   torch.istft(X, n_fft = W, hop_length = H, window = w, center = True, length = L) per row; W, H and the windows as in the
 *           forward transform.  Row b: frames[b] >= 1 frames, X complex64 [W/2+1][frames] (re, im interleaved) at COMPLEX element
 *           spec_off[b]; length[b] samples are written at out[out_off[b]]; length[b] = 0 (or length = NULL) means H (frames - 1), what torch
 *           returns without a length (nc_audio_istft_len; -1 on bad arguments).
 *   basis   T[n][j], n = 0..W-1, j = 0..W+1, evaluated in binary64 and rounded once, c_0 = c_{W/2} = 1 and c_k = 2 otherwise:
 *             T[n][2k] = fl(w(n) c_k cos(2 pi ((k n) mod W) / W) / W),  T[n][2k+1] = fl(-w(n) c_k sin(2 pi ((k n) mod W) / W) / W)
 *           and T[n][1] = T[n][W+1] = +0 exactly: the inverse real transform ignores the imaginary parts of bins 0 and W/2 (torch.istft of a
 *           spectrum with only those set is 0).  A NaN or an infinity there still poisons the frame, as 0 x NaN does.  (nc_audio_idft_basis)
 *   frame   y_t[n] = ONE chain over j ascending of fmaf(T[n][j], Xflat[j][t], acc) from acc = 0;  Xflat[2k] = re, Xflat[2k+1] = im.
 *   OLA     p = i + W/2 is the padded position of output sample i; frame t covers p where 0 <= p - t H < W.  Over the covering frames, t
 *           ascending:  num[i] = the binary32 sum of y_t[p - t H] from +0;  env[i] = fl(the binary64 sum of (double)w32(p - t H)^2 from 0),
 *           w32 = the window in binary64 rounded once;  out[i] = fl(num[i] / env[i]).  Samples with p >= W + H (frames - 1), a requested
 *           length past the covered span, are +0.  No floating-point atomics; a sample's value depends on nothing but its row.
 *           A result that is a NaN is stored as the quiet NaN 0x7fc00000 (hosts and gfx950 make different NaNs).
 *   NOLA    checked on the host before anything is launched (the envelope depends on W, H, the window, frames and the length only):
 *           NC_EINVAL where a covered output sample has a binary64 envelope <= 1e-11 (torch's rule); Hann with H = W is refused.
 *   groups  the frames go through a scratch of frames x W floats per row; the rows of a call run in groups whose scratch stays under a cap
 *           (256 MiB by default; a row above the cap is a group of its own, a row above 2 GiB is refused).  Grouping changes no bit.
 *           nc_audio_istft_workspace(device, set, &cap): set > 0 sets the cap in bytes, -1 restores the default, 0 keeps it; cap (nullable)
 *           receives the value in force.
 *   masks   nc_audio_spec_fill_*: per row the rectangle [k_lo, k_hi) x [t_lo, t_hi) of X [nbins][frames] is set to val exp(i val) =
 *           (fl(val cos val), fl(val sin val)), evaluated in binary64: (0, 0) for val = 0.  An empty rectangle writes nothing; a row may be
 *           named more than once.  One launch for all rows.  The index helpers restate the reference's interval test on a linspace:
 *             nc_audio_mask_freq_bins:   bin_hz[k] = k (sample_rate / 2) / (nbins - 1) in binary64 with the reference's INTEGER
 *               sample_rate / 2;  [k_lo, k_hi) = { k : fmin <= bin_hz[k] < fmax }, the float bounds widened
 *             nc_audio_mask_time_frames: bin_t[t] = t duration / (frames - 1), compared the same way
 *           (one bin or one frame: the only grid point is 0).  The reference's float32 linspace can differ from this exactly at a bin.
 *           Deviation from the reference: it sends every UNMASKED bin through abs / angle / exp, which moves it by a few ulp; here
 *           unmasked bins keep their bits.  fmin >= fmax or tmin >= tmax: NC_EINVAL (the reference throws).
 *   MFCC    mfcc[c][t] = ONE chain over m ascending of fmaf(dct[c][m], L[m][t], acc) from acc = 0,  L = nc_logf(fl(mel[m][t] + log_offset)),
 *           mel exactly what nc_audio_mel_spectrogram_* returns; a sum that is not finite gives L = NaN, and a NaN result is stored as
 *           0x7fc00000.  nc_logf: the natural logarithm on the ln(1 + f) core of nc_log10f (csrc/nc_math.h; its measured bound against
 *           binary64 is in tests/golden/spectral_bounds.json).  Output float [n_mfcc][frames] at out_off[b].
 *           dct[c][m] = fl(cos(pi c (2m + 1) / (2 n_mels)) sqrt(2 / n_mels)), row 0 times 1 / sqrt 2, in binary64: the orthonormal DCT-II
 *           (nc_audio_dct_matrix).  1 <= n_mfcc <= n_mels <= 512; log_offset a finite positive normal binary32.
 *           Deviation from the reference: its DCTMatrix ends in select(0, 0) and so returns ONE row of n_mels values, with which
 *           DSP.MFCC cannot produce n_mfcc coefficients; the evident intent (scale row 0) is built, tests/test_spectral_cpu.py
 *           transcribes the member as written and asserts what it yields.
 * All off[] / frames[] / length[] / k_*[] / t_*[] arrays are HOST arrays.
 * NC_EINVAL, before anything is launched: a null pointer (length excepted); B outside [1, 32767]; a negative offset or length;
 * frames[b] < 1; W, H or the window outside the forward transform's ranges; a NOLA failure; a rectangle outside [0, nbins] x
 * [0, frames]; nbins outside [1, 1025]; a fill value that is not finite; the MFCC ranges above and those of the mel spectrogram.
 *
 * replaces: DSP.InverseSTFT                          AudioTools/AudioTensorDSP.cs:124-151 as _dev (DEVICE buffers, asynchronous on
 *           `hip_stream`), plain (HOST buffers: upload, run, download) and _host (no device)
 * replaces: DSP.MaskFrequencies                      AudioTools/AudioTensorDSP.cs:307-345 (nc_audio_mask_freq_bins + nc_audio_spec_fill_*)
 * replaces: DSP.MaskTimesteps                        AudioTools/AudioTensorDSP.cs:356-394 (nc_audio_mask_time_frames + nc_audio_spec_fill_*)
 * replaces: DSP.MFCC                                 AudioTools/AudioTensorDSP.cs:408-441 with DCTMatrix (:901-912) */
NC_API int64_t nc_audio_istft_len(int64_t frames, int32_t W, int32_t H);
NC_API nc_status nc_audio_idft_basis(int32_t W, int32_t window, float* T /* [W][W+2] */);
NC_API nc_status nc_audio_istft_workspace(int device_index, int64_t set_bytes, int64_t* cap_bytes);
NC_API nc_status nc_audio_istft_dev(int device_index, const float* spec_c64, int32_t B, const int64_t* spec_off, const int64_t* frames, int32_t W,
                                    int32_t H, int32_t window, float* out, const int64_t* out_off, const int64_t* length, void* hip_stream);
NC_API nc_status nc_audio_istft(int device_index, const float* spec_c64, int32_t B, const int64_t* spec_off, const int64_t* frames, int32_t W,
                                int32_t H, int32_t window, float* out, const int64_t* out_off, const int64_t* length);
NC_API nc_status nc_audio_istft_host(const float* spec_c64, int32_t B, const int64_t* spec_off, const int64_t* frames, int32_t W, int32_t H,
                                     int32_t window, float* out, const int64_t* out_off, const int64_t* length);
NC_API nc_status nc_audio_mask_freq_bins(int32_t sample_rate, int32_t nbins, float fmin_hz, float fmax_hz, int32_t* k_lo, int32_t* k_hi);
NC_API nc_status nc_audio_mask_time_frames(float duration, int64_t frames, float tmin_s, float tmax_s, int64_t* t_lo, int64_t* t_hi);
NC_API nc_status nc_audio_spec_fill_dev(int device_index, float* spec_c64, int32_t B, const int64_t* spec_off, const int64_t* frames,
                                        int32_t nbins, const int32_t* k_lo, const int32_t* k_hi, const int64_t* t_lo, const int64_t* t_hi,
                                        float val, void* hip_stream);
NC_API nc_status nc_audio_spec_fill_host(float* spec_c64, int32_t B, const int64_t* spec_off, const int64_t* frames, int32_t nbins,
                                         const int32_t* k_lo, const int32_t* k_hi, const int64_t* t_lo, const int64_t* t_hi, float val);
NC_API nc_status nc_audio_dct_matrix(int32_t n_mfcc, int32_t n_mels, float* dct /* [n_mfcc][n_mels] */);
NC_API nc_status nc_audio_mfcc_dev(int device_index, const float* pcm, int32_t B, const int64_t* off, const int64_t* n, int32_t sample_rate,
                                   int32_t W, int32_t H, int32_t n_mels, float fmin, float fmax, int32_t n_mfcc, float log_offset, float* out,
                                   const int64_t* out_off, void* hip_stream);
NC_API nc_status nc_audio_mfcc_host(const float* pcm, int32_t B, const int64_t* off, const int64_t* n, int32_t sample_rate, int32_t W, int32_t H,
                                    int32_t n_mels, float fmin, float fmax, int32_t n_mfcc, float log_offset, float* out, const int64_t* out_off);

/* ------------------------------------------------------------------------------------ multi-GPU groups
 * The reference has no multi-device code; its callers batch clips (Examples/Program.cs:228-322, Models/Dia.cs:973-1002).  The path
 * shards over clips with no data-path exchange (every operator is per sample), so a group = one codec replica per GPU + ONE
 * collective: the RCCL all-gather of the emitted int64 codes (DAC [B,n_q,T'], SNAC.Encode's List<Tensor> as the levels of a clip side
 * by side: Models/SNAC.cs:129-150), issued on a side stream per device behind the encode, so the local decode overlaps it.
 * librccl is opened at run time by these entry points only.
 *   rank  mode: one process per GPU; rank 0 draws a unique id (nc_group_unique_id) and hands it to the others out of band.
 *   local mode: one process drives ndev GPUs (handles[i] created on device i): the natural layout of a single C# host process.
 * Lifetime: a group BORROWS its codec handles -- destroy the group (nc_group_destroy) before the codecs it was created over. */
typedef struct nc_group nc_group;
#define NC_GROUP_UID_BYTES 128
NC_API nc_status nc_group_unique_id(void* uid /* [NC_GROUP_UID_BYTES] */);
NC_API nc_status nc_group_create_rank(int32_t world, int32_t rank, const void* uid, nc_codec* local, nc_group** out);
NC_API nc_status nc_group_create_local(int32_t ndev, nc_codec* const* handles, nc_group** out);
/* local mode with options.  NC_GROUP_PEER_COPY: the all-gather is moved by peer copies (hipMemcpyPeerAsync on the members' side streams:
 * member e pulls slot d from member d's buffer behind d's "slot final" event) instead of RCCL -- same slots, same results, no librccl; the
 * members may then SHARE a device (an RCCL communicator cannot hold two ranks of one GPU), e.g. eight handles on one GPU split a batch
 * eight ways exactly as eight GPUs would.  flags = 0 is nc_group_create_local. */
#define NC_GROUP_PEER_COPY 1u
NC_API nc_status nc_group_create_local_ex(int32_t ndev, nc_codec* const* handles, uint32_t flags, nc_group** out);
NC_API nc_status nc_group_destroy(nc_group* g);
NC_API nc_status nc_group_info(const nc_group* g, int32_t* world, int32_t* rank /* -1 in local mode */);
/* Payload of the code all-gather: bits = 0 (default) moves the int64 codes as they are; 1..24 moves them bit-packed in the wire layout of
 * the reference's BitPacker (Modules/Encodec/BitPacker.cs: `bits` per value, LSB first, one packed row per clip; bits = 10 for 1024-entry
 * codebooks, 12 for SNAC's 4096) -- 64 / bits times fewer bytes on xGMI; pack and unpack run on the device around the collective and
 * the caller's tensors stay int64.  A code that does not fit `bits` is truncated to its low bits: pick bits >= log2(codebook size).
 * Rank mode: EVERY rank must set the same value before the next gather (the byte counts of the collective follow from it; a mismatch is
 * not detectable without another collective and hangs the gather). */
NC_API nc_status nc_group_set_code_bits(nc_group* g, int32_t bits);
/* rank mode, device pointers, asynchronous: encode this rank's B_local clips (nc_dac_encode_dev / nc_snac_encode_dev semantics) with the
 * codes written straight into slot `rank` of codes_all [world*B_local, ...], then the in-place all-gather on the group's side stream.
 * B_local must be the same on every rank (a ragged batch: pad the short shards to the longest one and drop the padding rows).
 * nc_group_wait makes the codec's stream wait for the gather (no host synchronisation). */
NC_API nc_status nc_group_dac_encode_allgather_dev(nc_group* g, const float* pcm, int32_t B_local, int64_t T, int32_t sample_rate, int32_t n_q,
                                                   int64_t* codes_all, float* z_local, float* latents_local);
NC_API nc_status nc_group_snac_encode_allgather_dev(nc_group* g, const float* pcm, int32_t B_local, int64_t T, int64_t* codes_all);
NC_API nc_status nc_group_wait(nc_group* g);
/* local mode, host pointers, synchronous: B_total clips split into contiguous blocks over the devices (the first B_total % ndev devices
 * hold one clip more; slots of the gathered buffer are sized for the largest block, so ragged batches gather in one collective);
 * codes [B_total, ...] come back gathered in clip order; z nullable [B_total, latent, T'] (each device returns its block).  One host
 * thread per device stages its block through pinned memory, so the uploads and encodes of all devices overlap. */
NC_API nc_status nc_group_dac_encode_allgather(nc_group* g, const float* pcm, int32_t B_total, int64_t T, int32_t sample_rate, int32_t n_q,
                                               int64_t* codes, float* z);
NC_API nc_status nc_group_snac_encode_allgather(nc_group* g, const float* pcm, int32_t B_total, int64_t T, int64_t* codes);
/* local mode, device pointers, asynchronous (the single-host layout of Examples/Program.cs:228-322 with the batch already split and
 * resident): pcm[d] [B_local[d],1,T] lives on member d's GPU and is encoded on member d's stream (nc_dac_encode_dev / nc_snac_encode_dev
 * semantics; z_local / latents_local nullable arrays of per-device outputs) with the codes written into slot d of codes_all[d], member
 * d's OWN copy of the gathered tensor [ndev * B_max, ...] (B_max = the largest block; a shorter block's slot is zero-padded); the grouped
 * in-place all-gather runs on the members' side streams, so every device ends up holding every block.  Nothing waits on the host:
 * nc_group_wait orders each codec's stream behind its gather; the decode of the local block can be queued before it. */
NC_API nc_status nc_group_dac_encode_allgather_local_dev(nc_group* g, const float* const* pcm, const int32_t* B_local, int64_t T,
                                                         int32_t sample_rate, int32_t n_q, int64_t* const* codes_all, float* const* z_local,
                                                         float* const* latents_local);
NC_API nc_status nc_group_snac_encode_allgather_local_dev(nc_group* g, const float* const* pcm, const int32_t* B_local, int64_t T,
                                                          int64_t* const* codes_all);

/* Encodec (Models/Encodec.cs:259-285: Encode emits one EncodedFrame per segment).  A rank's block is what nc_encodec_encode_dev writes: the
 * frames' code tensors [B_local, n_q, T'_f] end to end in segment order (n_q * sum T'_f values per clip) and scales [n_frames, B_local].
 * codes_all = [world][that block], scales_all = [world][n_frames][B_local] (nullable unless the model normalises): two collectives on the
 * side stream; rank r's frames are the views of block r.  Equal B_local everywhere.  nc_group_wait as above. */
NC_API nc_status nc_group_encodec_encode_allgather_dev(nc_group* g, const float* pcm, int32_t B_local, int64_t T, int64_t* codes_all,
                                                       float* scales_all);
NC_API nc_status nc_group_encodec_encode_allgather_local_dev(nc_group* g, const float* const* pcm, const int32_t* B_local, int64_t T,
                                                             int64_t* const* codes_all, float* const* scales_all);

/* ------------------------------------------------------------------------------------ profiling
 * Per-kernel-class timing with HIP events recorded on the handle's stream around every launch
 * (used by bench.py for the roofline object).  Classes are stable small integers. */
typedef enum {
    NC_KC_CONV_K7 = 0,   /* dilated k=7 residual-unit convolutions (MFMA implicit GEMM) */
    NC_KC_CONV_K1 = 1,   /* 1x1 channel-mix convolutions */
    NC_KC_CONV_DOWN = 2, /* strided down-sampling convolutions */
    NC_KC_CONV_UP = 3,   /* transposed (polyphase) up-sampling convolutions */
    NC_KC_CONV_MISC = 4, /* stem / head / k3 / decoder-input convolutions */
    NC_KC_RVQ = 5,       /* codebook argmin + gather kernels */
    NC_KC_ELEM = 6,      /* HBM-bound element-wise kernels: pooling, RVQ update, pad/activate, scale, embedding sum, overlap-add */
    NC_KC_DWCONV = 7,    /* depthwise k=7 convolutions (SNAC ResidualUnit.cs:25-60): 8 B per output */
    NC_KC_NORM = 8,      /* LayerNorm over channels (LocalMHA.cs:56) / GroupNorm(1,C) statistics (NormConv1d.cs:155) */
    NC_KC_ATTN = 9,      /* windowed rotary attention (LocalMHA.cs:84-113) */
    NC_KC_LSTM = 10,     /* LSTM recurrence (SLSTM.cs:40-57); the input projections are counted under conv_k1 */
    NC_KC_STEM = 11,     /* Cin <= 2 stem convolutions (Encoder.cs:31): a streaming store of Cout rows */
    NC_KC_HEAD = 12,     /* Cout <= 2 PCM-head convolutions (+tanh, Decoder.cs:44-46): a streaming read of Cin rows */
    NC_KC_COUNT = 13
} nc_kernel_class;

typedef struct {
    int64_t launches;
    double ms;          /* sum of event-to-event durations */
    double flops;       /* algorithmic flops of those launches (2*Cout*Cin/g*K*Tout*B) */
    double bytes;       /* algorithmic HBM bytes (input read once + output written once + weights once) */
} nc_profile_entry;

NC_API nc_status nc_codec_profile_enable(nc_codec* h, int32_t on);
NC_API nc_status nc_codec_profile_reset(nc_codec* h);
/* synchronises the stream, resolves pending events, fills out[NC_KC_COUNT] */
NC_API nc_status nc_codec_profile_read(nc_codec* h, nc_profile_entry* out);

/* ------------------------------------------------------------------------ op-level test hooks
 * Host-pointer, synchronous single-operator entry points over the same kernels the codecs use.
 * They exist so the parity tests can compare each HIP kernel with the oracle in isolation. */
typedef struct {
    int32_t B, Cin, Cout, K, stride, pad, dil, out_pad;
    int64_t Tin;
    int32_t transposed;      /* 0: conv1d weight [Cout,Cin,K]; 1: conv_transpose1d weight [Cin,Cout,K] */
    int32_t tanh_out;        /* apply tanh after bias/residual */
} nc_conv_desc;

/* y = epilogue(conv(snake_in?(x))), weight is the already-folded dense weight.
 * alpha_in [Cin] / alpha_out [Cout] / bias [Cout] / residual [B,Cout,Tout] are nullable. */
NC_API nc_status nc_op_conv1d(int device_index, const nc_conv_desc* d, const float* x, const float* weight, const float* bias,
                              const float* alpha_in, const float* alpha_out, const float* residual, float* y, int64_t* Tout);
/* Timing hook over the same launch path: runs the convolution `iters` times on device-resident seeded random data
 * (fuse bit0: Snake on input, bit1: Snake on output, bit2: residual add) and returns the HIP-event average per launch. */
NC_API nc_status nc_op_conv1d_bench(int device_index, const nc_conv_desc* d, int32_t fuse, int32_t iters, double* avg_ms);
/* One DAC ResidualUnit (ResidualUnit.cs:24-59): y = x + conv1(snake_a2(conv7_dil(snake_a1(x)))) on x [B,C,T].
 * Dense weights w7 [C,C,7], w1 [C,C,1].  fused != 0 requests the single-launch kernel (NC_EUNSUPPORTED when the shape has
 * none); iters > 0 additionally times `iters` repetitions with HIP events into *avg_ms (nullable when iters == 0). */
NC_API nc_status nc_op_res_unit(int device_index, int32_t B, int32_t C, int64_t T, int32_t dil, const float* x, const float* w7,
                                const float* b7, const float* a1, const float* a2, const float* w1, const float* b1,
                                int32_t fused, float* y, int32_t iters, double* avg_ms);
/* one VQ stage on projected latents z_e [B,D,T] against codebook [N,D] -> idx [B,T], st [B,D,T] */
NC_API nc_status nc_op_vq_argmin(int device_index, const float* z_e, int32_t B, int32_t D, int64_t T, const float* codebook,
                                 int32_t N, int64_t* idx, float* st);
/* the Encodec Euclidean RVQ (Modules/Encodec/ResidualVectorQuantizer.cs:133-157 over EuclideanCodebook.cs:155-182) on residual [B,D,T]
 * with codebooks [n_q,N,D] -> codes [B,n_q,T], residual_out [B,D,T] (nullable; the residual after the last stage in form 0, the input in form 1, whose residual never
 * leaves LDS).  form 0: one launch per stage; form 1: the all-stages matrix-core kernel (D == 128 and N = 512 or 1024, else NC_EUNSUPPORTED). */
NC_API nc_status nc_op_euclid_rvq(int device_index, const float* residual, int32_t B, int32_t D, int64_t T, const float* codebooks,
                                  int32_t n_q, int32_t N, int32_t form, int64_t* codes, float* residual_out);
/* The DAC quantizer (ResidualVectorQuantizer.cs:54-103 over VectorQuantizer.cs:67-125) on residual [B,L,T] through the routine the DAC
 * model's encode calls, on stage images built by the loader's routines from FOLDED dense weights: w_in [n_q,D,L], b_in [n_q,D] (nullable),
 * codebooks [n_q,N,D], w_out [n_q,L,D], b_out [n_q,L] (nullable) -> codes [B,n_q,T], zq [B,L,T], latents [B,n_q*D,T].  form 0: the launches
 * per stage (skinny in-projection, argmin, 1x1 convolution with the zq += q ; residual -= q epilogue); form 1: all stages in one launch,
 * NC_EUNSUPPORTED with nothing built or launched where that kernel has no instance (it wants D == 8, L in {256, 512, 768, 1024},
 * N % 64 == 0, N <= 1024).  form overrides NC_DAC_RVQ_STAGEWISE.  n_q <= 0: NC_EINVAL.  On an error the outputs are untouched. */
NC_API nc_status nc_op_dac_rvq(int device_index, const float* residual, int32_t B, int32_t L, int64_t T, int32_t n_q, int32_t N, int32_t D,
                               const float* w_in, const float* b_in, const float* codebooks, const float* w_out, const float* b_out,
                               int32_t form, int64_t* codes, float* zq, float* latents);
/* SNAC's quantizer update (ResidualVectorQuantizer.cs of SNAC: repeat_interleave of the stage's output at stride s): with q [rows,T/s],
 * zq [rows,T] = (first ? 0 : zq) + repeat(q, s) and, residual [rows,T] not null, residual -= repeat(q, s); both in place.  T % s == 0. */
NC_API nc_status nc_op_rvq_update(int device_index, const float* q, float* zq, float* residual, int64_t rows, int64_t T, int32_t s,
                                  int32_t first);
/* Code gather (VectorQuantizer.cs:135-142: Embedding + transpose): out[b,d,t] = codebook[code(b,t)][d] with code(b,t) =
 * codes[codes_offset + b * codes_bstride + t], codes a flat buffer of which the words up to codes_offset + (B-1) * codes_bstride + T are
 * read (SNAC keeps the levels of a clip side by side: codes_bstride > T).  A code outside [0, N) is CLAMPED to 0 or N - 1: that is the
 * engine's behaviour where the reference's Embedding would throw.  out points at [B,D,T] inside a buffer with out_guard floats in front
 * of it and out_guard behind; the whole buffer travels to the device and back, so a write outside [B,D,T] shows in the guards. */
NC_API nc_status nc_op_vq_gather(int device_index, const float* codebook, int32_t N, int32_t D, const int64_t* codes, int64_t codes_offset,
                                 int64_t codes_bstride, int32_t B, int64_t T, float* out, int64_t out_guard);
/* One activation of a loaded Encodec handle's SEANet stacks, as the driver holds it between launches (a "tap").  decoder == 0: the encoder
 * on x [B,channels,L] (no RMS normalisation); decoder != 0: the decoder on x [B,dimension,L].  The launches up to the tap are the ones
 * nc_encodec_encode / nc_encodec_decode make for a group of B rows.  Taps in driver order -- encoder: first conv | per stage: shortcut s,
 * branch h (k = 3), branch y (k = 1), down-conv | LSTM | last conv; decoder: first conv | LSTM | per stage: up-conv, s, h, y | last conv
 * (*n_taps = 3 + 4 * n_ratios).  out [B,C_out,L_out]: the tap with its pending GroupNorm applied, trimmed as its consumer reads it, without
 * the consumer's ELU; the LSTM tap is elu(x + lstm(x)).  stats [B][2] (nullable): (mean, rstd) of the tap's pending GroupNorm, written
 * where *has_stats comes back 1.  out == NULL: only *C_out, *L_out and *n_taps (tap < 0: only *n_taps); nothing is launched. */
NC_API nc_status nc_op_encodec_trace(nc_codec* h, int32_t decoder, const float* x, int32_t B, int64_t L, int32_t tap, float* out, float* stats,
                                     int32_t* C_out, int64_t* L_out, int32_t* n_taps, int32_t* has_stats);
/* One SLSTM stack of a loaded Encodec handle (SLSTM.forward, Modules/Encodec/SLSTM.cs:40-57; decoder == 0: the encoder's, else the
 * decoder's) on x [N,C,T] from GIVEN state, through the carried-state launcher of the causal streams (one fresh launch per time step;
 * the state rows are gathered from and scattered to a slot table by index): y [N,C,T] = elu?(x + lstm(x)) as the LSTM tap of
 * nc_op_encodec_trace, and h_state / c_state [N][layers][C] are read (nullable together: zero state) and overwritten with the state
 * behind step T - 1.  Host pointers, synchronous.  Splitting T into pieces and carrying the state gives the one-shot result bit for bit. */
NC_API nc_status nc_op_encodec_lstm_carried(nc_codec* h, int32_t decoder, const float* x, int32_t N, int64_t T, float* h_state, float* c_state,
                                            float* y);
/* The device copy every stream, session and ragged call is made of (concat_copy, csrc/nc_copy.h), alone: for each of n_desc descriptors
 * (a_off, na, b_off, nb, s0, dst_off, n) -- seven int64 each, in elements of elt = 4 or 8 bytes --
 * dst[dst_off + j] = (a[a_off, a_off + na) ++ b[b_off, b_off + nb) ++ zeros)[s0 + j] for j < n, all descriptors in ONE launch (n_desc <= 65535).
 * Host pointers, synchronous; dst [dst_n] is uploaded first, so what no descriptor covers comes back as it went in.  A descriptor that
 * leaves a [a_n], b [b_n] or dst is refused (NC_ESTATE) before anything is launched; destinations must not overlap. */
NC_API nc_status nc_op_concat_copy(int device_index, int32_t elt, const void* a, int64_t a_n, const void* b, int64_t b_n, void* dst, int64_t dst_n,
                                   const int64_t* desc, int64_t n_desc);
/* nc_log10f (csrc/nc_math.h, the canonical log10 of the quality metrics) on n positive normal binary32 values, evaluated on the host */
NC_API nc_status nc_op_log10f(const float* x, int64_t n, float* y);
/* nc_logf (csrc/nc_math.h, the canonical natural logarithm of the MFCC) on n positive normal binary32 values, evaluated on the host */
NC_API nc_status nc_op_logf(const float* x, int64_t n, float* y);
/* weight-norm fold w = v/(||v||+1e-7)*g over dim-0 slices (host-side, what load_weights does) */
NC_API nc_status nc_op_fold_weight_norm(const float* v, const float* g, int64_t d0, int64_t inner, float* w);
/* The HBM-bound SNAC kernels, one at a time (host pointers in and out, like nc_op_conv1d).
 * Depthwise convolution (ResidualUnit.cs:32, groups == C) on x [B,C,T], w [C][K], K <= 7: y [B,C,T] holds the first T outputs
 * y[b,c,t] = snake_out?(sum_k w[c,k] * snake_in?(x[b,c,t + k*dil - pad]) + bias[c]) over the zero-extended row; with "same" padding
 * (2*pad == dil*(K-1)) that is the whole convolution.  bias / alpha_in / alpha_out [C] are nullable. */
NC_API nc_status nc_op_dwconv1d(int device_index, int32_t B, int32_t C, int64_t T, int32_t K, int32_t pad, int32_t dil, const float* x,
                                const float* w, const float* bias, const float* alpha_in, const float* alpha_out, float* y);
/* LayerNorm over the channels of x [B,C,T] (LocalMHA.cs:85, eps 1e-5) -> y [B,C,T] */
NC_API nc_status nc_op_layer_norm(int device_index, int32_t B, int32_t C, int64_t T, const float* x, const float* gamma,
                                  const float* beta, float* y);
/* Windowed rotary attention (LocalMHA.cs:84-113) on qkv [B,3C,T] (channel = part*C + head*64 + d) -> y [B,C,T]; W <= 32, T % W == 0,
 * C % 64 == 0, else NC_EUNSUPPORTED.  inv_freq [32] is the checkpoint's rel_pos buffer (required); the cos / sin tables are built from it
 * by the function the SNAC model uses. */
NC_API nc_status nc_op_local_attn(int device_index, int32_t B, int32_t C, int64_t T, int32_t W, const float* qkv, const float* inv_freq,
                                  float* y);
/* avg_pool1d(s) (VectorQuantizer.cs:88) on x [rows,T] -> y [rows,T/s] */
NC_API nc_status nc_op_avg_pool(int device_index, int64_t rows, int64_t T, int32_t s, const float* x, float* y);
/* One depthwise SNAC ResidualUnit (ResidualUnit.cs:25-60): y = snake_next?(x + W1 . snake_a2(dw7_dil(snake_a1(x)) + b7) + b1) on x [B,C,T],
 * w7 [C][7], w1 [C][C]; b7 / b1 / alpha_next nullable.  fused != 0 runs the one-launch kernel whatever NC_SNAC_FUSE_MIN_COLS says and
 * returns NC_EUNSUPPORTED where that kernel does not serve the shape (it never falls back); fused == 0 runs the two-launch path. */
NC_API nc_status nc_op_snac_unit(int device_index, int32_t B, int32_t C, int64_t T, int32_t dil, const float* x, const float* w7,
                                 const float* b7, const float* a1, const float* a2, const float* w1, const float* b1,
                                 const float* alpha_next, int32_t fused, float* y);

#ifdef __cplusplus
}
#endif
#endif /* NC_MI355X_H */
