// C ABI (include/nc_mi355x.h): argument validation, exception -> status translation, host-buffer variants.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>

#include "nc_guard.h"

using namespace nc;


namespace {

template <class M, class Cfg>
nc_status create(const Cfg* cfg, int device_index, nc_codec** out) {
    return guard([&] {
        if (!cfg || !out) fail(NC_EINVAL, "cfg and out must not be null");
        *out = nullptr;
        std::unique_ptr<M> m(new M(*cfg));
        m->init_device(device_index);
        nc_codec* h = new nc_codec();
        h->impl = std::move(m);
        h->kind = M::kKind;
        *out = h;
    });
}

// A host-pointer call: `f` queues its copies and launches on the handle's own stream, whatever stream the device-pointer API was last
// bound to, and the caller's arrays are complete on return.
template <class F>
void on_own_stream(Codec& m, F&& f) {
    OwnStreamScope own(m);
    f();
    NC_HIP(hipStreamSynchronize(m.stream));
}

void h2d(void* d, const void* h, size_t n, hipStream_t s) { NC_HIP(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, s)); }
void d2h(void* h, const void* d, size_t n, hipStream_t s) { NC_HIP(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, s)); }

// A host-pointer Encodec call: `stage` queues the copies in, `run` the launch sequence on the staged arrays.  A timeout left behind by an
// EARLIER device-pointer call is not this call's failure: take note of it (step-wise LSTM kernels from here on) and carry on; that call's
// caller learns of it through nc_codec_check_errors / nc_codec_synchronize as documented.  A timeout of this call's own: run once more.
template <class Stage, class Run>
void encodec_host_call(EncodecModel& m, Stage&& stage, Run&& run) {
    m.lstm.note_timeout();
    stage();
    for (int attempt = 0;; ++attempt) {
        run();
        NC_HIP(hipStreamSynchronize(m.stream));
        if (!m.lstm.timed_out() || attempt) break;
        try { m.check_async_errors(); } catch (const Error&) {}   // clears the word, switches the handle to the step-wise LSTM: run again
    }
    m.check_async_errors();
}

// ---- helpers of the op-level test hooks ----
// The hooks build throw-away layers and buffers: all of them are DevBufs (or made of DevBufs) and go back to the device when the hook
// returns or throws.
float* op_upload(DevBuf& d, const float* h, size_t n) {
    d.reserve(n * 4);
    NC_HIP(hipMemcpy(d.p, h, n * 4, hipMemcpyHostToDevice));
    return d.as<float>();
}

// dense [B][C_in][T_in] -> [B][C_out][T_out]
ConvIO dense_io(const float* x, int C_in, int64_t T_in, float* y, int C_out, int64_t T_out) {
    ConvIO io{};
    io.x = x; io.x_bstride = (int64_t)C_in * T_in; io.x_cstride = T_in; io.x_len = (int32_t)T_in; io.Tin = T_in;
    io.y = y; io.y_bstride = (int64_t)C_out * T_out; io.y_cstride = T_out;
    return io;
}

// average milliseconds of fn() over `iters` calls on the null stream
template <class F>
double time_launches(int iters, F&& fn) {
    struct Event {
        hipEvent_t e = nullptr;
        Event() { NC_HIP(hipEventCreate(&e)); }
        ~Event() { (void)hipEventDestroy(e); }
    } e0, e1;
    NC_HIP(hipEventRecord(e0.e, nullptr));
    for (int i = 0; i < iters; ++i) fn();
    NC_HIP(hipEventRecord(e1.e, nullptr));
    NC_HIP(hipEventSynchronize(e1.e));
    float ms = 0.f;
    NC_HIP(hipEventElapsedTime(&ms, e0.e, e1.e));
    return (double)ms / iters;
}

}  // namespace

extern "C" {

const char* nc_last_error(void) { return get_last_error(); }
const char* nc_version(void) { return "nc_mi355x 0.1 (gfx950)"; }

const char* nc_debug_switches(void) { return env_switch_table(); }

int nc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

nc_status nc_dac_create(const nc_dac_config* cfg, int device_index, nc_codec** out) { return create<DacModel>(cfg, device_index, out); }

nc_status nc_codec_destroy(nc_codec* h) {
    return guard([&] {
        if (!h) return;
        if (h->impl) {
            h->impl->use_device();
            (void)hipStreamSynchronize(h->impl->stream);
        }
        delete h;
    });
}

nc_status nc_codec_load_weights_mem(nc_codec* h, const void* blob, size_t nbytes) {
    return guard([&] {
        Codec& m = codec_of(h);
        if (!blob) fail(NC_EINVAL, "blob must not be null");
        Blob b;
        b.parse(blob, nbytes);
        m.load(b);
    });
}

nc_status nc_blob_check(const void* blob, size_t nbytes, int32_t* n_tensors) {
    return guard([&] {
        if (!blob) fail(NC_EINVAL, "blob must not be null");
        Blob b;
        b.parse(blob, nbytes);
        if (n_tensors) *n_tensors = (int32_t)b.tensors.size();
    });
}

nc_status nc_codec_load_weights(nc_codec* h, const char* path) {
    return guard([&] {
        Codec& m = codec_of(h);
        if (!path) fail(NC_EINVAL, "path must not be null");
        std::ifstream f(path, std::ios::binary | std::ios::ate);
        if (!f) fail(NC_ENOTFOUND, "Weights not found at %s", path);  // DAC.cs:347-350 FileNotFoundException
        const std::streamsize n = f.tellg();
        f.seekg(0);
        std::vector<char> buf((size_t)n);
        if (!f.read(buf.data(), n)) fail(NC_ESTATE, "Failed to read weights from %s", path);
        Blob b;
        b.parse(buf.data(), buf.size());
        m.load(b);
    });
}

nc_status nc_codec_set_stream(nc_codec* h, void* hip_stream) {
    return guard([&] {
        codec_of(h).switch_stream(static_cast<hipStream_t>(hip_stream));
    });
}

nc_status nc_codec_reset_stream(nc_codec* h) {
    return guard([&] {
        Codec& m = codec_of(h);
        m.switch_stream(m.own_stream);
    });
}

nc_status nc_codec_synchronize(nc_codec* h) {
    return guard([&] {
        Codec& m = codec_of(h);
        m.use_device();
        NC_HIP(hipStreamSynchronize(m.stream));
        m.check_async_errors();
    });
}

nc_status nc_codec_check_errors(nc_codec* h) {
    return guard([&] {
        codec_of(h).check_async_errors();
    });
}

nc_status nc_encodec_lstm_stats(const nc_codec* h, int32_t* stepwise, int64_t* timeouts) {
    return guard([&] {
        EncodecModel& m = as<EncodecModel>(h);
        if (stepwise) *stepwise = m.lstm.force_stepwise ? 1 : 0;
        if (timeouts) *timeouts = m.lstm.timeouts;
    });
}

nc_status nc_dac_query(const nc_codec* h, int64_t T, int64_t* T_padded, int64_t* frames) {
    return guard([&] {
        DacModel& m = as<DacModel>(h);
        if (T <= 0) fail(NC_EINVAL, "T must be positive");
        if (T_padded) *T_padded = m.padded_len(T);
        if (frames) *frames = m.frames(T);
    });
}

nc_status nc_dac_encode_dev(nc_codec* h, const float* pcm, int32_t B, int64_t T, int32_t sample_rate, int32_t n_q, int64_t* codes,
                            float* z, float* latents) {
    return guard([&] { as<DacModel>(h).encode(false, pcm, B, T, sample_rate, n_q, codes, z, latents, nullptr); });
}

nc_status nc_dac_decode_dev(nc_codec* h, const float* z, int32_t B, int64_t frames, float* pcm) {
    return guard([&] { as<DacModel>(h).decode(false, z, nullptr, 0, B, frames, pcm); });
}

nc_status nc_dac_from_codes_dev(nc_codec* h, const int64_t* codes, int32_t B, int32_t n_q, int64_t frames, float* z) {
    return guard([&] { as<DacModel>(h).from_codes(false, codes, B, n_q, frames, z); });
}

nc_status nc_dac_encode(nc_codec* h, const float* pcm, int32_t B, int64_t T, int32_t sample_rate, int32_t n_q, int64_t* codes,
                        float* z, float* latents) {
    return guard([&] {
        DacModel& m = as<DacModel>(h);
        if (!pcm || !codes) fail(NC_EINVAL, "pcm and codes must not be null");
        if (B <= 0 || T <= 0) fail(NC_EINVAL, "B and T must be positive");
        on_own_stream(m, [&] { m.encode(true, pcm, B, T, sample_rate, n_q, codes, z, latents, nullptr); });
    });
}

nc_status nc_dac_decode(nc_codec* h, const float* z, int32_t B, int64_t frames, float* pcm) {
    return guard([&] {
        DacModel& m = as<DacModel>(h);
        if (!z || !pcm) fail(NC_EINVAL, "z and pcm must not be null");
        if (B <= 0 || frames <= 0) fail(NC_EINVAL, "B and frames must be positive");
        on_own_stream(m, [&] { m.decode(true, z, nullptr, 0, B, frames, pcm); });
    });
}

nc_status nc_dac_from_codes(nc_codec* h, const int64_t* codes, int32_t B, int32_t n_q, int64_t frames, float* z) {
    return guard([&] {
        DacModel& m = as<DacModel>(h);
        if (!codes || !z) fail(NC_EINVAL, "codes and z must not be null");
        if (B <= 0 || frames <= 0 || n_q <= 0) fail(NC_EINVAL, "bad codes shape");
        on_own_stream(m, [&] { m.from_codes(true, codes, B, n_q, frames, z); });
    });
}

nc_status nc_dac_from_latents_dev(nc_codec* h, const float* latents, int32_t B, int32_t C_lat, int64_t frames, float* z, float* projected,
                                  int64_t* codes) {
    return guard([&] { as<DacModel>(h).from_latents_dev(latents, B, C_lat, frames, z, projected, codes); });
}

// one upload, the device-pointer sequence on the staged arrays (which refuses what is to be refused before anything is queued), one
// download per output asked for
nc_status nc_dac_from_latents(nc_codec* h, const float* latents, int32_t B, int32_t C_lat, int64_t frames, float* z, float* projected,
                              int64_t* codes) {
    return guard([&] {
        DacModel& m = as<DacModel>(h);
        const int D = m.cfg.codebook_dim;
        if (!latents) fail(NC_EINVAL, "latents must not be null");
        if (!z && !projected && !codes) fail(NC_EINVAL, "z, projected and codes are all null: nothing to compute");
        if (B <= 0 || frames <= 0 || frames > ((int64_t)1 << 30)) fail(NC_EINVAL, "B and frames must be positive (at most 2^30 frames)");
        if (C_lat < D) fail(NC_EINVAL, "latents of %d channels hold no codebook of dimension %d", C_lat, D);
        if (!m.loaded) fail(NC_ESTATE, "weights not loaded (call nc_codec_load_weights first)");
        on_own_stream(m, [&] {
            const int n_q = std::min(m.cfg.n_codebooks, C_lat / D);
            const size_t n_in = (size_t)B * C_lat * frames * 4, n_z = (size_t)B * m.latent * frames * 4, n_pj = (size_t)B * n_q * D * frames * 4,
                         n_codes = (size_t)B * n_q * frames * 8;
            m.ck_in.reserve(n_in);
            if (z) m.ck_a.reserve(n_z);
            if (projected) m.ck_b.reserve(n_pj);
            if (codes) m.ck_codes.reserve(n_codes);
            h2d(m.ck_in.p, latents, n_in, m.stream);
            m.from_latents_dev(m.ck_in.as<float>(), B, C_lat, frames, z ? m.ck_a.as<float>() : nullptr, projected ? m.ck_b.as<float>() : nullptr,
                               codes ? m.ck_codes.as<int64_t>() : nullptr);
            if (z) d2h(z, m.ck_a.p, n_z, m.stream);
            if (projected) d2h(projected, m.ck_b.p, n_pj, m.stream);
            if (codes) d2h(codes, m.ck_codes.p, n_codes, m.stream);
        });
    });
}

nc_status nc_dac_decode_code_matrix_dev(nc_codec* h, const int64_t* codes_tq, int32_t B, int64_t frames, int32_t n_q, float* pcm) {
    return guard([&] { as<DacModel>(h).decode(false, nullptr, codes_tq, n_q, B, frames, pcm); });
}
nc_status nc_dac_encode_code_matrix_dev(nc_codec* h, const float* pcm, int32_t B, int64_t T, int32_t sample_rate, int64_t* codes_tq) {
    return guard([&] { as<DacModel>(h).encode(false, pcm, B, T, sample_rate, 0, nullptr, nullptr, nullptr, codes_tq); });
}
nc_status nc_dac_decode_code_matrix(nc_codec* h, const int64_t* codes_tq, int32_t B, int64_t frames, int32_t n_q, float* pcm) {
    return guard([&] {
        DacModel& m = as<DacModel>(h);
        if (!codes_tq || !pcm) fail(NC_EINVAL, "codes and pcm must not be null");
        if (B <= 0 || frames <= 0 || n_q <= 0) fail(NC_EINVAL, "bad code matrix shape");
        on_own_stream(m, [&] { m.decode(true, nullptr, codes_tq, n_q, B, frames, pcm); });
    });
}
nc_status nc_dac_encode_code_matrix(nc_codec* h, const float* pcm, int32_t B, int64_t T, int32_t sample_rate, int64_t* codes_tq) {
    return guard([&] {
        DacModel& m = as<DacModel>(h);
        if (!pcm || !codes_tq) fail(NC_EINVAL, "pcm and codes must not be null");
        if (B <= 0 || T <= 0) fail(NC_EINVAL, "B and T must be positive");
        on_own_stream(m, [&] { m.encode(true, pcm, B, T, sample_rate, 0, nullptr, nullptr, nullptr, codes_tq); });
    });
}

// ---- SNAC ------------------------------------------------------------------------------------------
nc_status nc_snac_create(const nc_snac_config* cfg, int device_index, nc_codec** out) { return create<SnacModel>(cfg, device_index, out); }

nc_status nc_snac_query(const nc_codec* h, int64_t T, int64_t* T_padded, int64_t* frames, int32_t* n_levels, int64_t* level_widths,
                        int64_t* decoded_len) {
    return guard([&] {
        SnacModel& m = as<SnacModel>(h);
        if (T <= 0) fail(NC_EINVAL, "T must be positive");
        const int64_t Tp = m.padded_len(T), Tz = Tp / m.hop;
        if (T_padded) *T_padded = Tp;
        if (frames) *frames = Tz;
        if (n_levels) *n_levels = m.cfg.n_vq_strides;
        if (level_widths)
            for (int i = 0; i < m.cfg.n_vq_strides; ++i) level_widths[i] = Tz / m.cfg.vq_strides[i];
        if (decoded_len) *decoded_len = m.decoded_len(Tz);
    });
}

nc_status nc_snac_noise_len(const nc_codec* h, int32_t B, int64_t frames, int64_t* n) {
    return guard([&] {
        SnacModel& m = as<SnacModel>(h);
        if (!n || B <= 0 || frames <= 0) fail(NC_EINVAL, "bad arguments");
        *n = m.noise_len(B, frames);
    });
}

nc_status nc_snac_encode_dev(nc_codec* h, const float* pcm, int32_t B, int64_t T, int64_t* codes, float* z, float* zq) {
    return guard([&] { as<SnacModel>(h).encode(false, pcm, B, T, codes, z, zq); });
}
nc_status nc_snac_encode_tensor_dev(nc_codec* h, const float* pcm, int32_t B, int64_t T, int64_t* codes, float* z, float* zq) {
    return guard([&] { as<SnacModel>(h).encode_dev(pcm, B, T, codes, z, zq, false); });
}
nc_status nc_snac_query_tensor(const nc_codec* h, int64_t T, int64_t* frames, int32_t* n_levels, int64_t* level_widths) {
    return guard([&] {
        SnacModel& m = as<SnacModel>(h);
        if (T <= 0) fail(NC_EINVAL, "T must be positive");
        const int64_t Tz = m.unpadded_frames(T);
        if (frames) *frames = Tz;
        if (n_levels) *n_levels = m.cfg.n_vq_strides;
        if (level_widths)
            for (int i = 0; i < m.cfg.n_vq_strides; ++i) level_widths[i] = Tz / m.cfg.vq_strides[i];
    });
}
nc_status nc_snac_from_codes_dev(nc_codec* h, const int64_t* codes, int32_t B, int64_t frames, float* zq) {
    return guard([&] { as<SnacModel>(h).from_codes(false, codes, B, frames, zq); });
}
nc_status nc_snac_decode_dev(nc_codec* h, const int64_t* codes, int32_t B, int64_t frames, const float* noise, uint64_t seed,
                             float* pcm) {
    return guard([&] { as<SnacModel>(h).decode(false, codes, B, frames, noise, seed, pcm); });
}

nc_status nc_snac_encode(nc_codec* h, const float* pcm, int32_t B, int64_t T, int64_t* codes, float* z, float* zq) {
    return guard([&] {
        SnacModel& m = as<SnacModel>(h);
        if (!pcm || !codes) fail(NC_EINVAL, "pcm and codes must not be null");
        if (B <= 0 || T <= 0) fail(NC_EINVAL, "B and T must be positive");
        on_own_stream(m, [&] { m.encode(true, pcm, B, T, codes, z, zq); });
    });
}

// the un-padded Tensor overload is never cut: one upload, the un-padded launch sequence, one download per output
nc_status nc_snac_encode_tensor(nc_codec* h, const float* pcm, int32_t B, int64_t T, int64_t* codes, float* z, float* zq) {
    return guard([&] {
        SnacModel& m = as<SnacModel>(h);
        if (!pcm || !codes) fail(NC_EINVAL, "pcm and codes must not be null");
        if (B <= 0 || T <= 0) fail(NC_EINVAL, "B and T must be positive");
        on_own_stream(m, [&] {
            const int64_t Tz = m.unpadded_frames(T);
            const size_t n_in = (size_t)B * T * 4, n_codes = (size_t)B * m.codes_per_clip(Tz) * 8, n_z = (size_t)B * m.latent * Tz * 4;
            m.ck_in.reserve(n_in); m.ck_codes.reserve(n_codes);
            if (z) m.ck_a.reserve(n_z);
            if (zq) m.ck_b.reserve(n_z);
            h2d(m.ck_in.p, pcm, n_in, m.stream);
            m.encode_dev(m.ck_in.as<float>(), B, T, m.ck_codes.as<int64_t>(), z ? m.ck_a.as<float>() : nullptr, zq ? m.ck_b.as<float>() : nullptr, false);
            d2h(codes, m.ck_codes.p, n_codes, m.stream);
            if (z) d2h(z, m.ck_a.p, n_z, m.stream);
            if (zq) d2h(zq, m.ck_b.p, n_z, m.stream);
        });
    });
}

nc_status nc_snac_from_codes(nc_codec* h, const int64_t* codes, int32_t B, int64_t frames, float* zq) {
    return guard([&] {
        SnacModel& m = as<SnacModel>(h);
        if (!codes || !zq) fail(NC_EINVAL, "codes and zq must not be null");
        if (B <= 0 || frames <= 0) fail(NC_EINVAL, "B and frames must be positive");
        on_own_stream(m, [&] { m.from_codes(true, codes, B, frames, zq); });
    });
}

nc_status nc_snac_decode(nc_codec* h, const int64_t* codes, int32_t B, int64_t frames, const float* noise, uint64_t seed,
                         float* pcm) {
    return guard([&] {
        SnacModel& m = as<SnacModel>(h);
        if (!codes || !pcm) fail(NC_EINVAL, "codes and pcm must not be null");   // ArgumentNullException, SNAC.cs:175
        if (B <= 0 || frames <= 0) fail(NC_EINVAL, "Codes list cannot be empty");   // ArgumentException, SNAC.cs:177-180
        on_own_stream(m, [&] { m.decode(true, codes, B, frames, noise, seed, pcm); });
    });
}

// SNAC.ProcessAudio (Models/SNAC.cs:255-282): resample (SNAC.cs:284-308) -> forward (:91-106) with the clip resident in HBM throughout.
nc_status nc_snac_process_audio_len(const nc_codec* h, int64_t n, int32_t sample_rate, int64_t* n_out) {
    return guard([&] {
        SnacModel& m = as<SnacModel>(h);
        if (!n_out) fail(NC_EINVAL, "n_out must not be null");
        if (n <= 0) fail(NC_EINVAL, "Audio data cannot be empty");
        if (sample_rate <= 0) fail(NC_EINVAL, "sample rate must be positive");
        *n_out = sample_rate == m.cfg.sample_rate ? n : nc_audio_resample_len(n, sample_rate, m.cfg.sample_rate);
    });
}

nc_status nc_snac_process_audio(nc_codec* h, const float* audio, int64_t n, int32_t sample_rate, const float* noise, uint64_t seed,
                                float* out) {
    return guard([&] {
        SnacModel& m = as<SnacModel>(h);
        if (!audio || n <= 0) fail(NC_EINVAL, "Audio data cannot be empty");   // ArgumentException, SNAC.cs:257-258
        if (!out) fail(NC_EINVAL, "out must not be null");
        if (sample_rate <= 0) fail(NC_EINVAL, "sample rate must be positive");
        on_own_stream(m, [&] {   // one clip, never cut: ck_a holds the raw audio of a resampled clip, ck_in the clip at the model's rate
            const bool resample = sample_rate != m.cfg.sample_rate;
            const int64_t T = resample ? nc_audio_resample_len(n, sample_rate, m.cfg.sample_rate) : n;
            if (T <= 0) fail(NC_EINVAL, "resampled clip would be empty");
            const int64_t Tz = m.padded_len(T) / m.hop;
            const size_t n_noise = (size_t)m.noise_len(1, Tz) * 4;
            m.ck_in.reserve((size_t)T * 4); m.ck_codes.reserve((size_t)m.codes_per_clip(Tz) * 8); m.ck_out.reserve((size_t)m.decoded_len(Tz) * 4);
            if (resample) {
                m.ck_a.reserve((size_t)n * 4);
                h2d(m.ck_a.p, audio, (size_t)n * 4, m.stream);
                const nc_status st = nc_audio_resample_linear_dev(m.device, m.ck_a.as<float>(), 1, n, sample_rate, m.cfg.sample_rate,
                                                                  m.ck_in.as<float>(), m.stream);
                if (st != NC_OK) fail(st, "%s", get_last_error());
            } else {
                h2d(m.ck_in.p, audio, (size_t)n * 4, m.stream);
            }
            const float* nz = nullptr;
            if (noise && n_noise) {
                m.ck_noise.reserve(n_noise);
                h2d(m.ck_noise.p, noise, n_noise, m.stream);
                nz = m.ck_noise.as<float>();
            }
            m.encode_dev(m.ck_in.as<float>(), 1, T, m.ck_codes.as<int64_t>(), nullptr, nullptr, true);
            m.decode_dev(m.ck_codes.as<int64_t>(), 1, Tz, nz, seed, m.ck_out.as<float>());
            d2h(out, m.ck_out.p, (size_t)T * 4, m.stream);                          // SNAC.cs:103 narrow(-1, 0, length)
        });
    });
}

// ---- Encodec ---------------------------------------------------------------------------------------
nc_status nc_encodec_create(const nc_encodec_config* cfg, int device_index, nc_codec** out) { return create<EncodecModel>(cfg, device_index, out); }

nc_status nc_encodec_set_bandwidth(nc_codec* h, float bw) {
    return guard([&] { as<EncodecModel>(h).set_bandwidth(bw); });
}

nc_status nc_encodec_query(const nc_codec* h, int64_t T, int32_t* n_frames, int32_t* n_q, int64_t* frame_lens, int32_t cap,
                           int64_t* decoded_len) {
    return guard([&] {
        EncodecModel& m = as<EncodecModel>(h);
        if (T <= 0) fail(NC_EINVAL, "T must be positive");
        const auto segs = m.segments(T);
        if (n_frames) *n_frames = (int32_t)segs.size();
        if (n_q) *n_q = m.n_q;
        if (frame_lens)
            for (size_t i = 0; i < segs.size() && (int32_t)i < cap; ++i) frame_lens[i] = segs[i].frames;
        if (decoded_len) *decoded_len = m.decoded_len(segs);
    });
}

nc_status nc_encodec_clip_length(const nc_codec* h, int32_t n_frames, const int64_t* frame_lens, int64_t* T) {
    return guard([&] {
        EncodecModel& m = as<EncodecModel>(h);
        if (!T || !frame_lens) fail(NC_EINVAL, "frame_lens and T must not be null");
        if (n_frames <= 0) fail(NC_EINVAL, "No frames provided to decode");                               // Encodec.cs:215-218
        const int64_t tail_frames = frame_lens[n_frames - 1];
        if (tail_frames <= 0) fail(NC_EINVAL, "a frame without codes");
        if (m.cfg.segment_length <= 0) {
            if (n_frames != 1) fail(NC_EINVAL, "Expected single frame when no segmentation is used");   // Encodec.cs:222-225
            for (int64_t L = std::max<int64_t>(1, (tail_frames - 2) * m.hop); L <= (tail_frames + 1) * m.hop; ++L)
                if (m.frames_for(L) == tail_frames) { *T = L; return; }
            fail(NC_EINVAL, "no clip length yields %lld frames", (long long)tail_frames);
        }
        const int64_t base = (int64_t)(n_frames - 1) * m.cfg.segment_stride;
        for (int64_t tail = 1; tail <= m.cfg.segment_stride; ++tail) {   // a longer tail would start another segment (Encodec.cs:278-282)
            if (m.frames_for(std::min<int64_t>(tail, m.cfg.segment_length)) != tail_frames) continue;
            const auto segs = m.segments(base + tail);                    // the segments before the last can be cut short by the clip end too
            bool same = (int32_t)segs.size() == n_frames;
            for (int32_t i = 0; same && i < n_frames; ++i) same = segs[(size_t)i].frames == frame_lens[i];
            if (same) { *T = base + tail; return; }
        }
        fail(NC_EINVAL, "no clip length yields this layout of %d segments (%lld frames in the last)", n_frames, (long long)tail_frames);
    });
}

nc_status nc_encodec_encode_dev(nc_codec* h, const float* pcm, int32_t B, int64_t T, int64_t* codes, float* scales, float* emb) {
    return guard([&] { as<EncodecModel>(h).encode_dev(pcm, B, T, codes, scales, emb); });
}
nc_status nc_encodec_decode_dev(nc_codec* h, const int64_t* codes, const float* scales, int32_t B, int64_t T, int32_t n_q, float* pcm) {
    return guard([&] { as<EncodecModel>(h).decode_dev(codes, scales, B, T, n_q, pcm); });
}

nc_status nc_encodec_encode(nc_codec* h, const float* pcm, int32_t B, int64_t T, int64_t* codes, float* scales, float* emb) {
    return guard([&] {
        EncodecModel& m = as<EncodecModel>(h);
        if (!pcm || !codes) fail(NC_EINVAL, "pcm and codes must not be null");                  // ArgumentNullException, Encodec.cs:245
        if (B <= 0 || T <= 0) fail(NC_EINVAL, "B and T must be positive");
        m.use_device();
        OwnStreamScope own(m);
        const auto segs = m.segments(T);
        int64_t fr = 0;
        for (auto& s : segs) fr += s.frames;
        const size_t n_in = (size_t)B * m.cfg.channels * T * 4, n_codes = (size_t)B * m.n_q * fr * 8, n_sc = segs.size() * (size_t)B * 4,
                     n_emb = (size_t)B * m.cfg.dimension * fr * 4;
        m.ck_in.reserve(n_in); m.ck_codes.reserve(n_codes); m.ck_a.reserve(n_sc); m.ck_b.reserve(n_emb);   // pcm, codes, scales, emb
        encodec_host_call(m, [&] { h2d(m.ck_in.p, pcm, n_in, m.stream); }, [&] {
            m.encode_dev(m.ck_in.as<float>(), B, T, m.ck_codes.as<int64_t>(), m.ck_a.as<float>(), emb ? m.ck_b.as<float>() : nullptr);
        });
        d2h(codes, m.ck_codes.p, n_codes, m.stream);
        if (scales && m.cfg.normalize) d2h(scales, m.ck_a.p, n_sc, m.stream);
        if (emb) d2h(emb, m.ck_b.p, n_emb, m.stream);
        NC_HIP(hipStreamSynchronize(m.stream));
    });
}

nc_status nc_encodec_decode(nc_codec* h, const int64_t* codes, const float* scales, int32_t B, int64_t T, int32_t n_q, float* pcm) {
    return guard([&] {
        EncodecModel& m = as<EncodecModel>(h);
        if (!codes || !pcm) fail(NC_EINVAL, "Invalid frame codes in Encodec Decode");              // Encodec.cs:438-442
        if (B <= 0 || T <= 0 || n_q <= 0) fail(NC_EINVAL, "No frames provided to decode");
        if (m.cfg.normalize && !scales) fail(NC_EINVAL, "this model normalises frames: scales must be given");
        m.use_device();
        OwnStreamScope own(m);
        const auto segs = m.segments(T);
        int64_t fr = 0;
        for (auto& s : segs) fr += s.frames;
        const int64_t Lout = m.decoded_len(segs);
        const size_t n_codes = (size_t)B * n_q * fr * 8, n_sc = segs.size() * (size_t)B * 4, n_out = (size_t)B * m.cfg.channels * Lout * 4;
        m.ck_codes.reserve(n_codes); m.ck_a.reserve(n_sc); m.ck_out.reserve(n_out);   // codes, scales, pcm
        encodec_host_call(m, [&] {
            h2d(m.ck_codes.p, codes, n_codes, m.stream);
            if (scales) h2d(m.ck_a.p, scales, n_sc, m.stream);
        }, [&] { m.decode_dev(m.ck_codes.as<int64_t>(), scales ? m.ck_a.as<float>() : nullptr, B, T, n_q, m.ck_out.as<float>()); });
        d2h(pcm, m.ck_out.p, n_out, m.stream);
        NC_HIP(hipStreamSynchronize(m.stream));
    });
}

nc_status nc_codec_profile_enable(nc_codec* h, int32_t on) {
    return guard([&] {
        codec_of(h).prof.on = on != 0;
    });
}

nc_status nc_codec_profile_reset(nc_codec* h) {
    return guard([&] {
        Codec& m = codec_of(h);
        m.use_device();
        m.prof.reset();
    });
}

nc_status nc_codec_profile_read(nc_codec* h, nc_profile_entry* out) {
    return guard([&] {
        if (!h || !h->impl || !out) fail(NC_EINVAL, "null argument");
        Codec& m = *h->impl;
        m.use_device();
        NC_HIP(hipStreamSynchronize(m.stream));
        m.prof.resolve();
        for (int i = 0; i < NC_KC_COUNT; ++i) out[i] = m.prof.acc[i];
    });
}

// ---- op-level test hooks -----------------------------------------------------------------------
nc_status nc_op_fold_weight_norm(const float* v, const float* g, int64_t d0, int64_t inner, float* w) {
    return guard([&] {
        if (!v || !g || !w || d0 <= 0 || inner <= 0) fail(NC_EINVAL, "bad arguments");
        fold_weight_norm_dac(v, g, d0, inner, w);
    });
}

nc_status nc_op_conv1d(int device_index, const nc_conv_desc* d, const float* x, const float* weight, const float* bias,
                       const float* alpha_in, const float* alpha_out, const float* residual, float* y, int64_t* Tout_p) {
    return guard([&] {
        if (!d || !x || !weight || !y) fail(NC_EINVAL, "null argument");
        if (d->B <= 0 || d->Cin <= 0 || d->Cout <= 0 || d->K <= 0 || d->stride <= 0 || d->Tin <= 0) fail(NC_EINVAL, "bad conv shape");
        use_checked_device(device_index);
        ConvLayer L;
        L.build(weight, bias, d->Cin, d->Cout, d->K, d->stride, d->pad, d->dil, d->out_pad, d->transposed != 0);
        const int64_t Tout = L.out_len(d->Tin);
        if (Tout <= 0) fail(NC_EINVAL, "empty output");
        if (Tout_p) *Tout_p = Tout;
        DevBuf dx, dy, dai, dao, dr;
        const size_t nx = (size_t)d->B * d->Cin * d->Tin, ny = (size_t)d->B * d->Cout * Tout;
        op_upload(dx, x, nx);
        dy.reserve(ny * 4);
        NC_HIP(hipMemset(dy.p, 0, ny * 4));
        ConvIO io = dense_io(dx.as<float>(), d->Cin, d->Tin, dy.as<float>(), d->Cout, Tout);
        io.alpha_in = alpha_in ? op_upload(dai, alpha_in, d->Cin) : nullptr;
        io.alpha_out = alpha_out ? op_upload(dao, alpha_out, d->Cout) : nullptr;
        io.res = residual ? op_upload(dr, residual, ny) : nullptr;
        io.epi = d->tanh_out ? EPI_TANH : 0;
        launch_conv(L, io, d->B, nullptr, nullptr);
        NC_HIP(hipDeviceSynchronize());
        NC_HIP(hipMemcpy(y, dy.p, ny * 4, hipMemcpyDeviceToHost));
    });
}

nc_status nc_op_conv1d_bench(int device_index, const nc_conv_desc* d, int32_t fuse, int32_t iters, double* avg_ms) {
    return guard([&] {
        if (!d || !avg_ms || iters <= 0) fail(NC_EINVAL, "null argument");
        if (d->B <= 0 || d->Cin <= 0 || d->Cout <= 0 || d->K <= 0 || d->stride <= 0 || d->Tin <= 0) fail(NC_EINVAL, "bad conv shape");
        use_checked_device(device_index);
        uint64_t st = 0x9E3779B97F4A7C15ull;
        auto rnd = [&]() {  // uniform [-1,1)
            st = st * 6364136223846793005ull + 1442695040888963407ull;
            return (float)((int64_t)(st >> 40) - (1 << 23)) * (1.0f / (1 << 23));
        };
        const size_t nw = (size_t)d->Cin * d->Cout * d->K;
        std::vector<float> w(nw), bias(d->Cout), al(std::max(d->Cin, d->Cout));
        const float sc = 1.0f / std::sqrt((float)d->Cin * (d->transposed ? 2 : d->K));
        for (auto& v : w) v = rnd() * sc;
        for (auto& v : bias) v = rnd() * 0.1f;
        for (auto& v : al) v = 1.25f + 0.75f * rnd();
        ConvLayer L;
        L.build(w.data(), bias.data(), d->Cin, d->Cout, d->K, d->stride, d->pad, d->dil, d->out_pad, d->transposed != 0);
        const int64_t Tout = L.out_len(d->Tin);
        if (Tout <= 0) fail(NC_EINVAL, "empty output");
        const size_t nx = (size_t)d->B * d->Cin * d->Tin, ny = (size_t)d->B * d->Cout * Tout;
        std::vector<float> hx(nx);
        for (auto& v : hx) v = rnd();
        DevBuf dx, dy, dai, dao, dr;
        op_upload(dx, hx.data(), nx); op_upload(dai, al.data(), al.size()); op_upload(dao, al.data(), al.size());
        dy.reserve(ny * 4); dr.reserve(ny * 4);
        NC_HIP(hipMemset(dr.p, 0, ny * 4));
        ConvIO io = dense_io(dx.as<float>(), d->Cin, d->Tin, dy.as<float>(), d->Cout, Tout);
        io.alpha_in = (fuse & 1) ? dai.as<float>() : nullptr;
        io.alpha_out = (fuse & 2) ? dao.as<float>() : nullptr;
        io.res = (fuse & 4) ? dr.as<float>() : nullptr;
        io.epi = d->tanh_out ? EPI_TANH : 0;
        // fuse & 8: Encodec GroupNorm block sums from the epilogue, finished in the launch; fuse & 16: Encodec input mode (pending
        // GroupNorm + ELU applied while staging)
        DevBuf gpart, gcnt, gstats, istats, igam;
        if (fuse & 8) {
            const int sub = conv_gn_sub(d->K, d->stride, d->Cout, d->transposed != 0);
            const int nrb = (int)(((int64_t)d->Cout * sub + 31) / 32), ncb = (int)(((Tout + sub - 1) / sub + 31) / 32);
            gpart.reserve((size_t)d->B * nrb * ncb * 16); gcnt.reserve((size_t)d->B * 4); gstats.reserve((size_t)d->B * 8);
            NC_HIP(hipMemset(gcnt.p, 0, (size_t)d->B * 4));
            if (!conv_gn_fusable(L, io)) fail(NC_EINVAL, "this layer cannot emit GroupNorm sums");
            io.gn_part = gpart.as<double>(); io.gn_nrb = nrb; io.gn_ncb = ncb;
            io.gn_count = gcnt.as<unsigned>(); io.gn_stats = gstats.as<float>(); io.gn_n = gn_count_arg((double)d->Cout * (double)Tout);
        }
        if (fuse & 16) {
            std::vector<float> st((size_t)d->B * 2), g((size_t)d->Cin * 2);
            for (int b = 0; b < d->B; ++b) { st[(size_t)2 * b] = 0.01f * rnd(); st[(size_t)2 * b + 1] = 1.0f + 0.1f * rnd(); }
            for (int c = 0; c < d->Cin; ++c) { g[(size_t)c] = 1.0f + 0.1f * rnd(); g[(size_t)d->Cin + c] = 0.1f * rnd(); }
            io.in_stats = op_upload(istats, st.data(), st.size());
            io.in_gamma = op_upload(igam, g.data(), g.size()); io.in_beta = io.in_gamma + d->Cin; io.in_elu = true;
        }
        for (int i = 0; i < 2; ++i) launch_conv(L, io, d->B, nullptr, nullptr);
        *avg_ms = time_launches(iters, [&] { launch_conv(L, io, d->B, nullptr, nullptr); });
    });
}

nc_status nc_op_res_unit(int device_index, int32_t B, int32_t C, int64_t T, int32_t dil, const float* x, const float* w7,
                         const float* b7, const float* a1, const float* a2, const float* w1, const float* b1, int32_t fused,
                         float* y, int32_t iters, double* avg_ms) {
    return guard([&] {
        if (!x || !w7 || !b7 || !a1 || !a2 || !w1 || !b1 || !y) fail(NC_EINVAL, "null argument");
        if (B <= 0 || C <= 0 || T <= 0 || dil <= 0 || iters < 0 || (iters > 0 && !avg_ms)) fail(NC_EINVAL, "bad arguments");
        use_checked_device(device_index);
        ConvLayer c7, c1;
        c7.build(w7, b7, C, C, 7, 1, 3 * dil, dil, 0, false);
        c1.build(w1, b1, C, C, 1, 1, 0, 1, 0, false);
        if (fused && !can_fuse_res_unit(c7, c1)) fail(NC_EUNSUPPORTED, "no fused residual-unit kernel for %d channels", C);
        const size_t n = (size_t)B * C * T;
        DevBuf dx, dh, dy, d1, d2;
        dh.reserve(n * 4); dy.reserve(n * 4);
        op_upload(dx, x, n); op_upload(d1, a1, C); op_upload(d2, a2, C);
        auto run = [&]() {
            ConvIO io = dense_io(dx.as<float>(), C, T, fused ? dy.as<float>() : dh.as<float>(), C, T);
            io.alpha_in = d1.as<float>(); io.alpha_out = d2.as<float>();
            if (fused) {
                io.res = dx.as<float>(); io.fuse_k1 = &c1;
                launch_conv(c7, io, B, nullptr, nullptr);
            } else {
                launch_conv(c7, io, B, nullptr, nullptr);
                ConvIO i2 = dense_io(dh.as<float>(), C, T, dy.as<float>(), C, T);
                i2.res = dx.as<float>();
                launch_conv(c1, i2, B, nullptr, nullptr);
            }
        };
        run();
        NC_HIP(hipDeviceSynchronize());
        NC_HIP(hipMemcpy(y, dy.p, n * 4, hipMemcpyDeviceToHost));
        if (iters > 0) *avg_ms = time_launches(iters, run);
    });
}

nc_status nc_op_vq_argmin(int device_index, const float* z_e, int32_t B, int32_t D, int64_t T, const float* codebook, int32_t N,
                          int64_t* idx, float* st) {
    return guard([&] {
        if (!z_e || !codebook || !idx || !st || B <= 0 || D <= 0 || T <= 0 || N <= 0) fail(NC_EINVAL, "bad arguments");
        use_checked_device(device_index);
        Codebook cb;
        cb.build(codebook, N, D);
        DevBuf dz, di, ds;
        const size_t nz = (size_t)B * D * T;
        op_upload(dz, z_e, nz);
        ds.reserve(nz * 4); di.reserve((size_t)B * T * 8);
        launch_vq_argmin(cb, dz.as<float>(), (int64_t)D * T, B, T, di.as<int64_t>(), T, ds.as<float>(), nullptr, nullptr);
        NC_HIP(hipDeviceSynchronize());
        NC_HIP(hipMemcpy(idx, di.p, (size_t)B * T * 8, hipMemcpyDeviceToHost));
        NC_HIP(hipMemcpy(st, ds.p, nz * 4, hipMemcpyDeviceToHost));
    });
}

nc_status nc_op_euclid_rvq(int device_index, const float* residual, int32_t B, int32_t D, int64_t T, const float* codebooks, int32_t n_q, int32_t N,
                           int32_t form, int64_t* codes, float* residual_out) {
    return guard([&] {
        if (!residual || !codebooks || !codes || B <= 0 || D <= 0 || T <= 0 || N <= 0 || n_q <= 0 || form < 0 || form > 1) fail(NC_EINVAL, "bad arguments");
        use_checked_device(device_index);
        op_euclid_rvq(residual, B, D, T, codebooks, n_q, N, form, codes, residual_out);
    });
}

nc_status nc_op_dac_rvq(int device_index, const float* residual, int32_t B, int32_t L, int64_t T, int32_t n_q, int32_t N, int32_t D,
                        const float* w_in, const float* b_in, const float* codebooks, const float* w_out, const float* b_out, int32_t form,
                        int64_t* codes, float* zq, float* latents) {
    return guard([&] {
        if (!residual || !w_in || !codebooks || !w_out || !codes || !zq || !latents) fail(NC_EINVAL, "null argument");
        if (B <= 0 || L <= 0 || T <= 0 || T > ((int64_t)1 << 30) || n_q <= 0 || n_q > 64 || N <= 0 || D <= 0 || form < 0 || form > 1 ||
            D > (1 << 20) || L > (1 << 20) || (int64_t)B * std::max<int64_t>(L, (int64_t)n_q * D) > ((int64_t)1 << 31) / T)
            fail(NC_EINVAL, "bad arguments");
        if (form == 1 && !dac_rvq_fused_admits(n_q, L, D, N))   // before anything is built or launched
            fail(NC_EUNSUPPORTED, "no one-launch DAC quantizer for latent %d, codebook %d x %d", L, N, D);
        use_checked_device(device_index);
        DacRvq rvq;
        for (int i = 0; i < n_q; ++i)
            rvq.add_stage(w_in + (size_t)i * D * L, b_in ? b_in + (size_t)i * D : nullptr, w_out + (size_t)i * L * D,
                          b_out ? b_out + (size_t)i * L : nullptr, codebooks + (size_t)i * N * D, L, D, N);
        rvq.upload_stages();
        const size_t nr = (size_t)B * L * T, nl = (size_t)B * n_q * D * T, nc = (size_t)B * n_q * T;
        DevBuf dr, dz, dl, dc, ds;
        op_upload(dr, residual, nr);
        dz.reserve(nr * 4); dl.reserve(nl * 4); dc.reserve(nc * 8); ds.reserve((size_t)B * D * T * 4);
        NC_HIP(hipMemset(dz.p, 0xFF, nr * 4));   // what a form leaves unwritten comes back as NaN / -1
        NC_HIP(hipMemset(dl.p, 0xFF, nl * 4));
        NC_HIP(hipMemset(dc.p, 0xFF, nc * 8));
        rvq.quantize(form, n_q, L, D, N, dr.as<float>(), B, T, dc.as<int64_t>(), dz.as<float>(), dl.as<float>(), ds.as<float>(), nullptr, nullptr);
        NC_HIP(hipDeviceSynchronize());
        NC_HIP(hipMemcpy(codes, dc.p, nc * 8, hipMemcpyDeviceToHost));
        NC_HIP(hipMemcpy(zq, dz.p, nr * 4, hipMemcpyDeviceToHost));
        NC_HIP(hipMemcpy(latents, dl.p, nl * 4, hipMemcpyDeviceToHost));
    });
}

nc_status nc_op_rvq_update(int device_index, const float* q, float* zq, float* residual, int64_t rows, int64_t T, int32_t s, int32_t first) {
    return guard([&] {
        if (!q || !zq) fail(NC_EINVAL, "null argument");
        if (rows <= 0 || T <= 0 || s <= 0 || T % s != 0 || rows > ((int64_t)1 << 31) / T) fail(NC_EINVAL, "bad update shape");
        use_checked_device(device_index);
        const size_t n = (size_t)rows * T;
        DevBuf dq, dz, dr;
        op_upload(dq, q, n / s); op_upload(dz, zq, n);
        float* r = residual ? op_upload(dr, residual, n) : nullptr;
        launch_rvq_update(dq.as<float>(), dz.as<float>(), r, rows, T, s, first != 0, nullptr, nullptr);
        NC_HIP(hipDeviceSynchronize());
        NC_HIP(hipMemcpy(zq, dz.p, n * 4, hipMemcpyDeviceToHost));
        if (residual) NC_HIP(hipMemcpy(residual, dr.p, n * 4, hipMemcpyDeviceToHost));
    });
}

nc_status nc_op_vq_gather(int device_index, const float* codebook, int32_t N, int32_t D, const int64_t* codes, int64_t codes_offset,
                          int64_t codes_bstride, int32_t B, int64_t T, float* out, int64_t out_guard) {
    return guard([&] {
        if (!codebook || !codes || !out) fail(NC_EINVAL, "null argument");
        if (N <= 0 || D <= 0 || B <= 0 || T <= 0 || T > ((int64_t)1 << 30) || codes_offset < 0 || codes_bstride < T || out_guard < 0 ||
            codes_bstride > ((int64_t)1 << 31) / B || (int64_t)B * D > ((int64_t)1 << 31) / T)
            fail(NC_EINVAL, "bad gather shape");
        use_checked_device(device_index);
        Codebook cb;
        cb.build(codebook, N, D);
        const size_t n_codes = (size_t)codes_offset + (size_t)(B - 1) * codes_bstride + T;   // the words the B rows of T codes span
        const size_t n_out = (size_t)B * D * T + 2 * (size_t)out_guard;
        DevBuf dc, dout;
        dc.reserve(n_codes * 8);
        NC_HIP(hipMemcpy(dc.p, codes, n_codes * 8, hipMemcpyHostToDevice));
        op_upload(dout, out - out_guard, n_out);
        launch_vq_gather(cb, dc.as<int64_t>() + codes_offset, codes_bstride, B, T, dout.as<float>() + out_guard, nullptr, nullptr);
        NC_HIP(hipDeviceSynchronize());
        NC_HIP(hipMemcpy(out - out_guard, dout.p, n_out * 4, hipMemcpyDeviceToHost));
    });
}

nc_status nc_op_encodec_trace(nc_codec* h, int32_t decoder, const float* x, int32_t B, int64_t L, int32_t tap, float* out, float* stats,
                              int32_t* C_out, int64_t* L_out, int32_t* n_taps, int32_t* has_stats) {
    return guard([&] {
        EncodecModel& m = as<EncodecModel>(h);
        if (n_taps) *n_taps = m.trace_taps();
        if (tap < 0 && !out) return;                                   // the tap count alone
        if (B <= 0 || L <= 0) fail(NC_EINVAL, "B and L must be positive");
        int C = 0; int64_t Lt = 0;
        m.trace_shape(decoder != 0, L, tap, &C, &Lt);
        if (C_out) *C_out = C;
        if (L_out) *L_out = Lt;
        if (!out) return;                                              // sizes only: nothing is launched
        if (!x) fail(NC_EINVAL, "x must not be null");
        m.use_device();
        OwnStreamScope own(m);
        const size_t n_in = (size_t)B * (decoder ? m.cfg.dimension : m.cfg.channels) * L * 4, n_out = (size_t)B * C * Lt * 4;
        m.ck_in.reserve(n_in);
        const float* st = nullptr;
        const float* y = nullptr;
        encodec_host_call(m, [&] { h2d(m.ck_in.p, x, n_in, m.stream); }, [&] { y = m.trace_dev(decoder != 0, m.ck_in.as<float>(), B, L, tap, &st); });
        d2h(out, y, n_out, m.stream);
        if (has_stats) *has_stats = st ? 1 : 0;
        if (stats && st) d2h(stats, st, (size_t)B * 2 * 4, m.stream);
        NC_HIP(hipStreamSynchronize(m.stream));
    });
}

// ---- op hooks over the HBM-bound SNAC kernels (nc_elem.hip, nc_snac_unit.hip) ----

nc_status nc_op_dwconv1d(int device_index, int32_t B, int32_t C, int64_t T, int32_t K, int32_t pad, int32_t dil, const float* x,
                         const float* w, const float* bias, const float* alpha_in, const float* alpha_out, float* y) {
    return guard([&] {
        if (!x || !w || !y) fail(NC_EINVAL, "null argument");
        if (B <= 0 || C <= 0 || T <= 0 || T > ((int64_t)1 << 30) || K <= 0 || pad < 0 || dil <= 0) fail(NC_EINVAL, "bad depthwise shape");
        use_checked_device(device_index);
        DwConvLayer L;
        L.build(w, bias, C, K, pad, dil);
        DevBuf dx, dy, dai, dao;
        const size_t n = (size_t)B * C * T;
        op_upload(dx, x, n);
        dy.reserve(n * 4);
        NC_HIP(hipMemset(dy.p, 0, n * 4));
        const float* ai = alpha_in ? op_upload(dai, alpha_in, C) : nullptr;
        const float* ao = alpha_out ? op_upload(dao, alpha_out, C) : nullptr;
        launch_dwconv(L, dx.as<float>(), ai, ao, dy.as<float>(), B, T, nullptr, nullptr);
        NC_HIP(hipDeviceSynchronize());
        NC_HIP(hipMemcpy(y, dy.p, n * 4, hipMemcpyDeviceToHost));
    });
}

nc_status nc_op_layer_norm(int device_index, int32_t B, int32_t C, int64_t T, const float* x, const float* gamma, const float* beta, float* y) {
    return guard([&] {
        if (!x || !gamma || !beta || !y) fail(NC_EINVAL, "null argument");
        if (B <= 0 || C <= 0 || T <= 0) fail(NC_EINVAL, "bad LayerNorm shape");
        use_checked_device(device_index);
        DevBuf dx, dy, dg, db;
        const size_t n = (size_t)B * C * T;
        op_upload(dx, x, n); op_upload(dg, gamma, C); op_upload(db, beta, C);
        dy.reserve(n * 4);
        NC_HIP(hipMemset(dy.p, 0, n * 4));
        launch_layernorm_ct(dx.as<float>(), dg.as<float>(), db.as<float>(), dy.as<float>(), B, C, T, nullptr);
        NC_HIP(hipDeviceSynchronize());
        NC_HIP(hipMemcpy(y, dy.p, n * 4, hipMemcpyDeviceToHost));
    });
}

nc_status nc_op_local_attn(int device_index, int32_t B, int32_t C, int64_t T, int32_t W, const float* qkv, const float* inv_freq, float* y) {
    return guard([&] {
        if (!qkv || !inv_freq || !y) fail(NC_EINVAL, "null argument");
        if (B <= 0 || C <= 0 || T <= 0) fail(NC_EINVAL, "bad attention shape");
        if (W <= 0 || W > 32 || T % W != 0 || C % 64 != 0) fail(NC_EUNSUPPORTED, "local attention: window %d / dim %d / %lld steps not supported", W, C, (long long)T);
        use_checked_device(device_index);
        std::vector<float> cs, sn;
        rotary_tables(inv_freq, W, cs, sn);
        DevBuf dq, dy, dc, ds;
        const size_t n = (size_t)B * C * T;
        op_upload(dq, qkv, 3 * n); op_upload(dc, cs.data(), cs.size()); op_upload(ds, sn.data(), sn.size());
        dy.reserve(n * 4);
        NC_HIP(hipMemset(dy.p, 0, n * 4));
        launch_local_attn(dq.as<float>(), dc.as<float>(), ds.as<float>(), dy.as<float>(), B, C, T, W, nullptr);
        NC_HIP(hipDeviceSynchronize());
        NC_HIP(hipMemcpy(y, dy.p, n * 4, hipMemcpyDeviceToHost));
    });
}

nc_status nc_op_avg_pool(int device_index, int64_t rows, int64_t T, int32_t s, const float* x, float* y) {
    return guard([&] {
        if (!x || !y) fail(NC_EINVAL, "null argument");
        if (rows <= 0 || T <= 0 || s <= 0 || T / s <= 0) fail(NC_EINVAL, "bad pooling shape");
        use_checked_device(device_index);
        DevBuf dx, dy;
        const size_t ny = (size_t)rows * (size_t)(T / s);
        op_upload(dx, x, (size_t)rows * T);
        dy.reserve(ny * 4);
        NC_HIP(hipMemset(dy.p, 0, ny * 4));
        launch_avg_pool(dx.as<float>(), dy.as<float>(), rows, T, s, nullptr);
        NC_HIP(hipDeviceSynchronize());
        NC_HIP(hipMemcpy(y, dy.p, ny * 4, hipMemcpyDeviceToHost));
    });
}

nc_status nc_op_snac_unit(int device_index, int32_t B, int32_t C, int64_t T, int32_t dil, const float* x, const float* w7, const float* b7,
                          const float* a1, const float* a2, const float* w1, const float* b1, const float* alpha_next, int32_t fused,
                          float* y) {
    return guard([&] {
        if (!x || !w7 || !a1 || !a2 || !w1 || !y) fail(NC_EINVAL, "null argument");
        if (B <= 0 || C <= 0 || T <= 0 || T > ((int64_t)1 << 30) || dil <= 0) fail(NC_EINVAL, "bad arguments");
        use_checked_device(device_index);
        DevBuf dx, dh, dy, d1, d2, dn;
        const size_t n = (size_t)B * C * T;
        op_upload(dx, x, n);
        dy.reserve(n * 4);
        NC_HIP(hipMemset(dy.p, 0, n * 4));
        const float* an = alpha_next ? op_upload(dn, alpha_next, C) : nullptr;
        SnacFusedUnit fu;   // the layers of either form outlive the synchronisation below
        DwConvLayer dw;
        ConvLayer c1;
        if (fused) {
            if (!SnacFusedUnit::supported(C, 7, dil)) fail(NC_EUNSUPPORTED, "no one-launch SNAC unit for %d channels at dilation %d", C, dil);
            fu.build(C, dil, w7, b7, a1, a2, w1, b1);
            if (!fu.usable(dx.as<float>(), dy.as<float>(), T, B, /*any_cols=*/true))   // the caller chose this form: no column threshold
                fail(NC_EUNSUPPORTED, "the one-launch SNAC unit does not serve this call: %lld steps (it wants a multiple of 4, >= 256, C * T < 2^30), or NC_SNAC_NO_FUSE is set", (long long)T);
            hipDeviceProp_t prop;
            NC_HIP(hipGetDeviceProperties(&prop, device_index));
            fu.launch(dx.as<float>(), an, dy.as<float>(), B, T, prop.multiProcessorCount, nullptr, nullptr);
        } else {
            dw.build(w7, b7, C, 7, 3 * dil, dil);
            c1.build(w1, b1, C, C, 1, 1, 0, 1, 0, false);
            dh.reserve(n * 4);
            launch_dwconv(dw, dx.as<float>(), op_upload(d1, a1, C), op_upload(d2, a2, C), dh.as<float>(), B, T, nullptr, nullptr);
            ConvIO io = dense_io(dh.as<float>(), C, T, dy.as<float>(), C, T);
            io.res = dx.as<float>(); io.alpha_out = an;
            launch_conv(c1, io, B, nullptr, nullptr);
        }
        NC_HIP(hipDeviceSynchronize());
        NC_HIP(hipMemcpy(y, dy.p, n * 4, hipMemcpyDeviceToHost));
    });
}

}  // extern "C"
