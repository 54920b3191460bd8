// Engine objects behind the opaque nc_codec handle.
#pragma once
#include <functional>
#include <memory>

#include "nc_common.h"
#include "nc_conv.h"
#include "nc_elem.h"
#include "nc_lstm.h"

namespace nc {

const char* get_last_error();
void fold_weight_norm_dac(const float* v, const float* g, int64_t d0, int64_t inner, float* w);
void fold_weight_norm_snac(const float* v, const float* g, int64_t d0, int64_t inner, float* w);
inline void upload_f32(DevBuf& d, const float* h, size_t n) {   // n floats of the host into d, grown to hold them
    d.reserve(n * sizeof(float));
    NC_HIP(hipMemcpy(d.p, h, n * sizeof(float), hipMemcpyHostToDevice));
}

// ---- RVQ kernels (nc_rvq.hip) ----------------------------------------------------------------
// Codebook resident on the device in the two layouts the kernels want.
struct Codebook {
    int N = 0, D = 0;
    DevBuf cbT;  // [D][N] transposed copy: conflict-free LDS image for the argmin
    DevBuf cb;   // [N][D] row-major: gather
    DevBuf c2;   // [N] squared norms (canonical fma chain, computed once on the host)
    void build(const float* host_cb, int N, int D);
};
// One stage of the stage-fused DAC quantizer (nc_rvq.hip): dense projection weights beside the codebook images, all device pointers.
struct RvqStage {
    const float* w_inT;   // [latent][D]  in_proj weight, transposed (folded weight norm)
    const float* b_in;    // [D]
    const float* w_out;   // [latent][D]  out_proj weight
    const float* b_out;   // [latent]
    const float* cbT;     // [D][N]
    const float* c2;      // [N]
    const float* cb;      // [N][D]
};
// The shapes the one-launch kernel has an instantiation for: D == 8, L in {256, 512, 768, 1024}, N a multiple of 64 up to 1024, n_q >= 1
bool dac_rvq_fused_admits(int n_q, int L, int D, int N);
// ResidualVectorQuantizer.forward for n_q stages in ONE launch (ResidualVectorQuantizer.cs:54-103); returns false, with nothing
// launched, when the shape has no instantiation (the caller then runs the stage-by-stage launches).  residual [B,L,T] (read only),
// zq [B,L,T], latents [B,n_q*D,T], codes [B,n_q,T].
bool launch_dac_rvq_fused(const RvqStage* stages_dev, int n_q, int L, int D, int N, const float* residual, int B, int64_t T, int64_t* codes,
                          float* zq, float* latents, hipStream_t s, Profiler* prof);
// z_e [B,D,T] (batch stride ze_bstride) -> codes[b*codes_bstride + t] (int64) and st [B,D,T] = z_e + (cb[idx] - z_e)
void launch_vq_argmin(const Codebook& cb, const float* z_e, int64_t ze_bstride, int B, int64_t T, int64_t* codes,
                      int64_t codes_bstride, float* st, hipStream_t s, Profiler* prof);
// codes -> out [B,D,T] = cb[codes]  (Embedding + transpose, VectorQuantizer.cs:135-142)
void launch_vq_gather(const Codebook& cb, const int64_t* codes, int64_t codes_bstride, int B, int64_t T, float* out, hipStream_t s,
                      Profiler* prof);

// The DAC quantizer resident on the device (nc_dac.hip): per stage the packed projection layers of the stage-by-stage launches, the
// codebook images and the dense projection weights of the one-launch kernel.  DacModel is one, filled by its loader; the test hook
// nc_op_dac_rvq fills one from host arrays through the same routines.
struct DacRvq {
    std::vector<std::unique_ptr<ConvLayer>> in_proj, out_proj;
    std::vector<std::unique_ptr<Codebook>> codebooks;
    std::vector<std::unique_ptr<DevBuf>> rvq_dense;   // dense projection weights / biases of the stage-fused quantizer
    DevBuf rvq_stages;                                // RvqStage[stages]
    void clear_stages();
    // the next stage from folded dense weights: w_in [D][L], w_out [L][D], codebook [N][D]; b_in [D] / b_out [L] nullable (then zero)
    void add_stage(const float* w_in, const float* b_in, const float* w_out, const float* b_out, const float* codebook, int L, int D, int N);
    void upload_stages();                             // after the last add_stage
    // ResidualVectorQuantizer.forward, first n_q stages (ResidualVectorQuantizer.cs:54-103): residual [B,L,T] (updated in place by the
    // stage-by-stage form) -> codes [B,n_q,T], zq [B,L,T], latents [B,n_q*D,T]; st: workspace of B*D*T floats.  form < 0: one launch
    // where the shape has the instance and NC_DAC_RVQ_STAGEWISE is unset, else a launch sequence per stage; form 0 / 1 force the
    // stage-by-stage / the one-launch form whatever the environment says (1 fails with NC_EUNSUPPORTED on a shape it does not take).
    void quantize(int form, int n_q, int L, int D, int N, float* residual, int B, int64_t T, int64_t* codes, float* zq, float* latents,
                  float* st, hipStream_t s, Profiler* prof);

  private:
    std::vector<RvqStage> stage_tab;
};

// ---- Euclidean RVQ of Encodec (nc_euclid_rvq.hip) ----------------------------------------------
constexpr int EUCLID_MAX_D = 128;   // widest code vector the kernels hold in LDS
// The stages' codebooks as the kernels take them: device pointers per stage on the host (cb [N][D], cbT [D][N], c2 [N]) and as device arrays
struct EuclidBooks {
    int N = 0, D = 0;
    std::vector<const float*> cb, cbT, c2;
    DevBuf d_cb, d_cbT, d_c2;
    void add(const Codebook& b);   // the next stage (all stages share N and D)
    void upload();                 // after the last add
};
// ResidualVectorQuantizer.Encode (:133-157), first n_q stages: residual [B,D,T] -> codes [B,n_q,T].  form < 0: all stages in one matrix-core
// launch where the shape has the instance (D == 128, N = 512 or 1024) and NC_EUCLID_NO_MFMA is unset, else one launch per stage (updates the
// residual in place); form 0 / 1 force the per-stage / the matrix-core form (which fails on a shape it does not take).
void launch_euclid_rvq(const EuclidBooks& bk, int n_q, int form, float* residual, int B, int64_t T, int64_t* codes, hipStream_t s);
// ResidualVectorQuantizer.Decode (:107-124): codes [B,n_q,T] -> emb [B,D,T], the stages' code vectors added in ascending order
void launch_emb_sum(const EuclidBooks& bk, const int64_t* codes, int n_q, int B, int64_t T, float* emb, hipStream_t s);
// Test hook (nc_op_euclid_rvq): the quantizer on host arrays, residual [B,D,T] and n_q codebooks [n_q][N][D]; form as above, 0 or 1
void op_euclid_rvq(const float* residual_in, int B, int D, int64_t T, const float* books_host, int n_q, int N, int form, int64_t* codes_host, float* residual_out);

// ---- codec objects ---------------------------------------------------------------------------
// How one call is cut along the frame axis (nc_chunk.hip).  n_chunks == 1: the window is the clip.
struct ChunkPlan {
    int64_t n_chunks = 1, chunk = 0, halo_l = 0, halo_r = 0;
    int64_t arena_bytes = 0;
};
enum ChunkKind { CK_ENCODE = 0, CK_DECODE = 1, CK_FROM_CODES = 2 };
void launch_copy_rows(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows, hipStream_t s);

struct Codec {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    bool loaded = false;
    int cu_count = 0;              // compute units of the device (multiProcessorCount)
    size_t lds_per_cu = 0;         // LDS a workgroup may opt into (maxSharedMemoryPerMultiProcessor)
    Profiler prof;
    // nc_chunk.hip: NC_CHUNK_AUTO (0) / NC_CHUNK_OFF (-1) / chunk size in latent frames, and the dense per-window buffers (grow-only).
    // They are the staging buffers of every host-pointer call too: a clip that is not cut is one window.
    int64_t chunk_frames = 0;
    DevBuf ck_in, ck_codes, ck_a, ck_b, ck_out, ck_noise, ck_noise_full;
    // nc_ragged.hip: kept width C and rows per launch batch of the ragged calls (0 = default), the descriptor tables of one call (pinned
    // host image, device copy, the event behind the copy), the packed tensors of a host-pointer call and the drawn noise of all clips
    int64_t ragged_kept = 0;
    int32_t ragged_max_windows = 0;
    struct RaggedTables {
        DevBuf dev;
        void* pin = nullptr;
        size_t pin_cap = 0;
        hipEvent_t ev = nullptr;
        bool ev_used = false;
        ~RaggedTables();
    } rg_tab;
    DevBuf rg_in, rg_out, rg_noise;
    // rows x width bytes between two pitched arrays on `stream`; either side may be a host pointer (then a 2-D memcpy), device to
    // device is the copy kernel of nc_util.hip.  All sizes are multiples of 4 bytes.
    void copy2d(void* dst, bool dst_host, size_t dpitch, const void* src, bool src_host, size_t spitch, size_t width, size_t rows);
    virtual ~Codec();
    virtual void load(const Blob& blob) = 0;
    void init_device(int device_index);
    void use_device() const;
    // errors raised by device code after the launch returned (bounded spins of the persistent kernels): called once the stream is idle
    virtual void check_async_errors() {}
    // Rebind the handle to another stream.  The workspaces are shared by all calls on the handle, so work already queued on the old
    // stream is ordered before anything the new stream will launch (event record + wait; no host synchronisation).
    void switch_stream(hipStream_t s);
};

// Host-pointer entry points run on the handle's own stream whatever stream the device-pointer API was last bound to.
struct OwnStreamScope {
    Codec& c;
    hipStream_t prev;
    explicit OwnStreamScope(Codec& c_) : c(c_), prev(c_.stream) { c.use_device(); c.switch_stream(c.own_stream); }
    ~OwnStreamScope() {
        try { c.switch_stream(prev); } catch (...) {}
    }
};

struct DacModel : Codec, DacRvq {
    static constexpr int kKind = 0;
    static constexpr const char* kKindName = "a DAC";
    nc_dac_config cfg{};
    int latent = 0, hop = 1;
    bool fuse_res_units = true;  // NC_NO_FUSE=1 in the environment selects the two-launch residual units (A/B, tests)

    struct ResUnit {
        DevBuf a1, a2;
        ConvLayer c7, c1;
    };
    ConvLayer enc_stem;
    struct EncBlk {
        ResUnit ru[3];
        DevBuf a_down;
        ConvLayer down;
    } enc[8];
    DevBuf enc_alpha_out;
    ConvLayer enc_out;

    // the quantizer's stages: DacRvq (in_proj, out_proj, codebooks, rvq_stages)

    ConvLayer dec_in;
    struct DecBlk {
        DevBuf a_up;
        ConvLayer up;
        ResUnit ru[3];
    } dec[8];
    DevBuf dec_alpha_out;
    ConvLayer dec_out;

    // workspace (grow-only)
    DevBuf act[3], resid, zq, lat, st, codes_ws;
    // nc_dia.hip: the reverted codes in the packed ragged layout and the decoded PCM in front of the speed adjustment (grow-only)
    DevBuf dia_codes, dia_pcm;

    explicit DacModel(const nc_dac_config& c);
    void load(const Blob& blob) override;
    int64_t padded_len(int64_t T) const { return (T + hop - 1) / hop * hop; }
    int64_t frames(int64_t T) const { return (T + hop - 1) / hop; }
    int64_t decoded_len(int64_t frames) const;
    // the launch sequences on device pointers (async on `stream`)
    void encode_dev(const float* pcm, int B, int64_t T, int sample_rate, int n_q, int64_t* codes, float* z, float* latents);
    void decode_dev(const float* z, int B, int64_t frames, float* pcm);
    void from_codes_dev(const int64_t* codes, int B, int n_q, int64_t frames, float* z);
    // nc_dac_latents.hip: latents [B,C_lat,frames] -> z [B,latent,frames], projected [B,n_q*D,frames], codes [B,n_q,frames] with
    // n_q = min(n_codebooks, C_lat / D); any output may be null, not all three
    void from_latents_dev(const float* latents, int B, int C_lat, int64_t frames, float* z, float* projected, int64_t* codes);
    void decode_code_matrix_dev(const int64_t* codes_tq, int B, int64_t frames, int n_q, float* pcm);
    void encode_code_matrix_dev(const float* pcm, int B, int64_t T, int sample_rate, int64_t* codes_tq);
    // The operations of the C ABI (nc_chunk.hip), async on `stream`.  `host`: the caller's arrays are host pointers.  Each plans the
    // call and runs the launch sequence above window by window through the ck_* buffers; a device-pointer call that is not cut is the
    // launch sequence on the caller's own arrays.  encode: codes / z / latents or, with codes_tq, Dia's [B, T', n_q] matrix of all
    // codebooks; decode: from z or, with codes_tq, from such a matrix.
    ChunkPlan chunk_plan(ChunkKind kind, int B, int64_t frames) const;
    // activation arena of the launch sequence `kind` on B rows of W frames (3 rotating buffers of the widest tensor)
    static int64_t arena_bytes(const nc_dac_config& cfg, ChunkKind kind, int64_t B, int64_t W);
    void encode(bool host, const float* pcm, int B, int64_t T, int sample_rate, int n_q, int64_t* codes, float* z, float* latents, int64_t* codes_tq);
    void decode(bool host, const float* z, const int64_t* codes_tq, int n_q, int B, int64_t frames, float* pcm);
    void from_codes(bool host, const int64_t* codes, int B, int n_q, int64_t frames, float* z);

  private:
    float* run_res_unit(ResUnit& ru, int dil, float* cur, int C, int64_t L, int B, int& cur_idx, const float* alpha_next);
};

struct SnacModel : Codec {
    static constexpr int kKind = 1;
    static constexpr const char* kKindName = "a SNAC";
    nc_snac_config cfg{};
    int latent = 0, hop = 1;
    int64_t pad_to = 1;

    struct ResUnit {
        DevBuf a1, a2;
        DwConvLayer dw;   // depthwise flavour
        ConvLayer c7;     // dense flavour (depthwise == 0)
        ConvLayer c1;
        SnacFusedUnit fu; // depthwise flavour, narrow long rows: the whole unit in one launch
    };
    struct Mha {
        int C = 0;
        DevBuf gamma, beta, cs, sn;
        ConvLayer qkv, out;
    };
    ConvLayer enc_stem;
    struct EncBlk {
        ResUnit ru[3];
        DevBuf a_down;
        ConvLayer down;
    } enc[8];
    Mha enc_mha, dec_mha;
    DwConvLayer enc_out_dw, dec_in_dw;
    ConvLayer enc_out, dec_in;

    std::vector<std::unique_ptr<ConvLayer>> in_proj, out_proj;
    std::vector<std::unique_ptr<Codebook>> codebooks;

    struct DecBlk {
        DevBuf a_up;
        ConvLayer up, noise;
        ResUnit ru[3];
    } dec[8];
    DevBuf dec_alpha_out;
    ConvLayer dec_out;

    DevBuf act[3], resid, zq, pooled, qbuf, lat, st, qkv_ws, noise_ws;

    explicit SnacModel(const nc_snac_config& c);
    void load(const Blob& blob) override;
    int64_t padded_len(int64_t T) const { return (T + pad_to - 1) / pad_to * pad_to; }
    static int64_t up_len(int64_t L, int s) { return (L - 1) * s - 2 * ((s + 1) / 2) + 2 * s + (s % 2); }
    int64_t decoded_len(int64_t frames) const;
    int64_t noise_len(int B, int64_t frames) const;
    int64_t codes_per_clip(int64_t frames) const {
        int64_t n = 0;
        for (int i = 0; i < cfg.n_vq_strides; ++i) n += frames / cfg.vq_strides[i];
        return n;
    }
    // pad = true: SNAC.Encode(float[]) / forward (Preprocess, then the encoder on the padded tensor; SNAC.cs:129-150, 91-106)
    // pad = false: SNAC.Encode(Tensor) AS WRITTEN (SNAC.cs:113-122, deviation D7): the encoder runs on the un-padded tensor
    void encode_dev(const float* pcm, int B, int64_t T, int64_t* codes, float* z, float* zq, bool pad = true);
    // frames the encoder emits for an un-padded row of T samples; NC_EINVAL where the reference's quantizer / LocalMHA would throw
    int64_t unpadded_frames(int64_t T) const;
    void from_codes_dev(const int64_t* codes, int B, int64_t frames, float* zq);
    void decode_dev(const int64_t* codes, int B, int64_t frames, const float* noise, uint64_t seed, float* pcm);
    // the operations of the C ABI (nc_chunk.hip), as DacModel's; encode is the padded form
    ChunkPlan chunk_plan(ChunkKind kind, int B, int64_t frames) const;
    static int64_t arena_bytes(const nc_snac_config& cfg, ChunkKind kind, int64_t B, int64_t W);
    void encode(bool host, const float* pcm, int B, int64_t T, int64_t* codes, float* z, float* zq);
    void from_codes(bool host, const int64_t* codes, int B, int64_t frames, float* zq);
    void decode(bool host, const int64_t* codes, int B, int64_t frames, const float* noise, uint64_t seed, float* pcm);

  private:
    // n frames of every code level from frame s0 of src ([B][codes_per_clip(Ts)]) to frame d0 of dst ([B][codes_per_clip(Td)])
    void copy_levels(int64_t* dst, bool dst_host, int64_t Td, int64_t d0, const int64_t* src, bool src_host, int64_t Ts, int64_t s0, int64_t n, int B);
    void load_res_unit(const Blob& b, const std::string& q, ResUnit& ru, int C, int dil);
    void load_mha(const Blob& b, const std::string& p, Mha& m, int C);
    float* run_res_unit(ResUnit& ru, float* cur, int C, int64_t L, int B, int& cur_idx, const float* alpha_next);
    float* run_mha(Mha& m, float* cur, int C, int64_t L, int B, int& cur_idx, const float* alpha_next);
    void reserve_act(int B, int64_t Tp);
};

struct EncodecModel : Codec {
    static constexpr int kKind = 2;
    static constexpr const char* kKindName = "an Encodec";
    nc_encodec_config cfg{};
    int hop = 1, n_q = 1;

    struct SConv {                 // SConv1d / SConvTranspose1d: conv (+ GroupNorm affine when time_group_norm)
        int K = 0, stride = 1, Cin = 0, Cout = 0;
        bool transposed = false;
        ConvLayer conv;
        DevBuf gamma, beta;
    };
    struct ResBlock { SConv c1, c2, sc; };
    struct Plan { int64_t left = 0, right = 0, Lz = 0, Lp = 0, Lout = 0; };
    struct Seg { int64_t off = 0, len = 0, frames = 0; };
    struct Act {                   // [N,C,L] view of a raw conv output + its pending GroupNorm
        const float* p = nullptr;
        int C = 0;
        int64_t L = 0, rs = 0, off = 0;
        const float* stats = nullptr;
        const float* gamma = nullptr;
        const float* beta = nullptr;
    };

    SConv enc_in, enc_down[8], enc_out, dec_in, dec_up[8], dec_out;
    ResBlock enc_res[8], dec_res[8];
    Lstm enc_lstm, dec_lstm;
    std::vector<std::unique_ptr<Codebook>> books;
    EuclidBooks book_tab;                        // their pointer tables (nc_euclid_rvq.hip)

    std::vector<std::unique_ptr<DevBuf>> pool;   // per-call intermediates, same allocation order every call (grow-only)
    size_t pool_i = 0;
    // A ragged call runs many batches per stream: it splits the pool into one lane per stream (pool_lanes = 3, buffer i of lane l is
    // pool[3 i + l]) and every batch starts over at the head of its lane, so the arena is bounded by the largest batch.  Batches of one
    // lane are ordered by their stream.  Every other call runs with one lane: pool[pool_i], as ever.
    int pool_lanes = 1, pool_lane = 0;
    LstmRuntime lstm{*this};                     // timeout word, ticket, second stream and events of the LSTM launches (nc_lstm.hip)
    // segment groups of one call are independent until the overlap-add: the first runs on the handle's stream, the others on side
    // streams (forked / joined with events), so the short tail segment of a clip hides behind the full-length batch
    hipStream_t side_stream[2] = {nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[2] = {nullptr, nullptr};
    // overlap-add operands (decode_dev): the window and the weight sum depend on the frame geometry only and stay on the device;
    // the per-call frame pointers travel through a small ring of pinned host slots, so decode_dev never synchronises the stream
    struct Ola {
        std::vector<int64_t> key;
        DevBuf w, sw;
        void* pin = nullptr;
        size_t slot_bytes = 0;
        int next = 0;
        hipEvent_t ev[4] = {};
        bool ev_used[4] = {};
    } ola;
    bool on_side_group = false;
    ~EncodecModel() override;

    explicit EncodecModel(const nc_encodec_config& c);
    void check_async_errors() override;
    void load(const Blob& blob) override;
    void set_bandwidth(float bw);
    Plan plan_sconv(int64_t L, int k, int stride, int dil) const;
    int64_t frames_for(int64_t L) const;
    int64_t decoded_for(int64_t Tz) const;
    std::vector<Seg> segments(int64_t T) const;
    int64_t decoded_len(const std::vector<Seg>& segs) const {   // samples of the clip decoded from these segments (overlap-add at segment_stride)
        return cfg.segment_length <= 0 ? decoded_for(segs[0].frames)
                                       : (int64_t)cfg.segment_stride * ((int64_t)segs.size() - 1) + decoded_for(segs.back().frames);
    }
    void encode_dev(const float* pcm, int B, int64_t T, int64_t* codes, float* scales, float* emb);
    void decode_dev(const int64_t* codes, const float* scales, int B, int64_t T, int nq, float* pcm);
    // Ragged batches (nc_encodec_ragged.hip): the segments of B clips of unequal lengths pooled into uniform batches of at most
    // ragged_rows rows (0 = default).  Device pointers, async on `stream`; lengths is a host array of clip lengths in samples.
    int32_t ragged_rows = 0;
    static constexpr int RAGGED_MAX_ROWS = 4096;   // = GN_MAX_SAMPLES: one arrival counter per row of a batch
    DevBuf rg_frames;               // decoded frames of all batches of a ragged decode, alive until its one overlap-add launch
    void encode_ragged_dev(const float* pcm, int B, const int64_t* lengths, int64_t* codes, float* scales, float* emb);
    void decode_ragged_dev(const int64_t* codes, const float* scales, int B, const int64_t* lengths, int nq, float* pcm);
    // Stream pool (nc_encodec_stream.hip): segments of live streams pooled into the same batches; its steps call encode_batch / decode_batch
    friend struct ::nc_encodec_stream_pool;
    // Causal streams (nc_encodec_causal.hip): windows of live streams through encoder_front / decoder_tail, the LSTM from carried state
    friend struct ::nc_encodec_causal_pool;
    float* alloc(size_t n_floats);   // the next buffer of the pool (of the running batch's lane), grown to n_floats
    // Test hook (nc_op_encodec_trace).  A tap is every activation view the driver holds between launches, numbered in the order the
    // driver produces them: encoder = first conv | per stage: shortcut s, branch h, branch y, down-conv | LSTM | last conv; decoder =
    // first conv | LSTM | per stage: up-conv, s, h, y | last conv.  The LSTM tap is elu(x + lstm(x)).
    int trace_taps() const { return 3 + 4 * cfg.n_ratios; }
    // channels and length of tap `tap` for rows of L samples (encoder) or frames (decoder): host arithmetic on the pad plans; raises what the stack raises
    void trace_shape(bool decoder, int64_t L, int tap, int* C_out, int64_t* L_out) const;
    // Runs the encoder stack (no RMS normalisation) or the decoder stack on the dense device tensor x [N, channels | dimension, L] up to
    // tap `tap` -- the launches encode_batch / decode_batch make -- and returns the tap as a dense device tensor [N, C, L_tap]: pending
    // GroupNorm applied, trimmed, no ELU.  *stats: the tap's [N][2] (mean, rstd) on the device, null where no GroupNorm is pending.
    const float* trace_dev(bool decoder, const float* x, int N, int64_t L, int tap, const float** stats);

  private:
    void load_sconv(const Blob& b, const std::string& key, SConv& L, int Cin, int Cout, int K, int stride, bool transposed);
    void load_resblock(const Blob& b, const std::string& key, ResBlock& r, int dim);
    float* pad_act(const Act& a, const Act* b2, bool elu, int N, const Plan& pl);
    struct GnJob { bool on = false, fused = false, finished = false; int sub = 1, nrb = 0, ncb = 0; double* part = nullptr; float* stats = nullptr; };
    static constexpr int GN_MAX_SAMPLES = 4096;   // rows of a segment group (encode_dev caps a group at 4096)
    static_assert(RAGGED_MAX_ROWS == GN_MAX_SAMPLES, "a ragged batch is a segment group");
    DevBuf gn_counters;                           // [3 groups][2][GN_MAX_SAMPLES] arrival counters of the in-launch GroupNorm finish (zero between launches; the second set: the
                                                  // branch output of the fused first pass of a residual block, two outputs finishing in one launch)
    int cur_group = 0;
    unsigned* group_counters() { return gn_counters.as<unsigned>() + (size_t)cur_group * 2 * GN_MAX_SAMPLES; }   // the running segment group's set
    bool gn_finishes_in_launch(int N) const;      // GroupNorm sums emitted by a launch over N rows can be finished inside it
    GnJob gn_begin(const ConvLayer& conv, ConvIO& io, int N, int C, int64_t L, int sub);
    const float* gn_end(const GnJob& j, const float* raw, int N, int C, int64_t L, int64_t rs = 0);   // rs: row pitch of `raw` (0 = dense rows of L)
    // the streaming two-input kernels in front of sconv / sconvT: false = not this shape (nothing launched)
    bool try_stream_down(SConv& L, const Act& a, const Act* b2, bool elu, int N, const Plan& pl, Act& out);
    bool try_stream_up(SConv& L, const Act& a, const Act* b2, bool elu, int N, Act& out);
    Act sconv(SConv& L, const Act& a, const Act* b2, bool elu, int N);
    Act sconvT(SConv& L, const Act& a, const Act* b2, bool elu, int N);
    void resblock(ResBlock& r, const Act& x, int N, Act& s, Act& y);
    bool resblock_first_pass(ResBlock& r, const Act& x, int N, Act& s, Act& h);   // shortcut + k = 3 branch in one launch (nc_resa.hip); false: not this shape
    float* materialize(const Act& a, int N, const float* scale, int mode);
    // body(first, G) per group of consecutive segments with equal `key` (at most 4096 rows): the first on the handle's stream, the others on side streams
    template <class Body>
    void for_each_group(const std::vector<Seg>& segs, int B, int64_t Seg::*key, Body&& body);
    // body(i) per independent batch i, on lane lanes[i]: 0 = the handle's stream, 1 / 2 = the side streams (forked from and joined to the
    // handle's stream with events; each lane has its own set of gn_counters).  lane_pools: every batch allocates from the head of its lane.
    void run_batches(const std::vector<int>& lanes, bool lane_pools, const std::function<void(size_t)>& body);
    void ola_tables(const std::vector<int64_t>& flen, int64_t stride, int64_t total);
    char* ola_stage(const std::vector<const float*>& fp, const std::vector<int64_t>& flen);
    void encode_batch(const float* x, int N, int64_t L, int64_t Tz, int64_t* codes, float* scale_out, float* emb_out);
    float* decode_batch(const int64_t* codes, int N, int nq, int64_t Tz, const float* scale, int64_t* Lout);
    Act encoder_stack(Act cur, int N);                        // SEANetEncoder.forward on an activation view -> the last conv's pending view
    Act encoder_front(Act cur, int N);                        // ... its convolutional front: up to the LSTM's input (pending view)
    Act decoder_tail(Act s, bool lstm_elu, int N);            // SEANetDecoder.forward behind the LSTM: up-stack and last conv on the LSTM's output s
    Act decoder_stack(const float* emb, int N, int64_t Tz);   // SEANetDecoder.forward on dense emb [N,dimension,Tz]
    // the tap of trace_dev: with no trace running (want < 0, every production call) tap() is one compare
    struct TapReached {};
    struct Trace { int want = -1, n = 0; bool lstm = false, lstm_has_elu = false; Act act; } trace;
    void tap(const Act& a, bool lstm = false, bool lstm_has_elu = false) {
        if (trace.want < 0) return;
        if (trace.n++ == trace.want) { trace.act = a; trace.lstm = lstm; trace.lstm_has_elu = lstm_has_elu; throw TapReached{}; }
    }
};

}  // namespace nc

// the opaque handle of the C ABI
struct nc_codec {
    std::unique_ptr<nc::Codec> impl;
    int kind = 0;  // the model's kKind
};
