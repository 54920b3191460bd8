// The SLSTM of Encodec (nc_lstm.hip): the weights of a stack and the per-handle state of its launch sequence.
#pragma once
#include <memory>

#include "nc_common.h"
#include "nc_conv.h"

namespace nc {

struct EncodecModel;
struct LstmTicket;   // per-device serialisation of persistent LSTM sections across handles (nc_lstm.hip)

struct LstmLayer { ConvLayer ih; DevBuf whh, whhp, bhh, bih; };
struct Lstm { int C = 0; std::vector<std::unique_ptr<LstmLayer>> layers; };
// the `n_layers` layers of the stack under `key` (weight_ih / weight_hh / bias_ih / bias_hh _l<i>), with the A-fragment image of W_hh
void load_lstm(const Blob& b, const std::string& key, Lstm& l, int C, int n_layers);
// true when LstmRuntime::run should apply the consumer's ELU in its output store (NC_LSTM_NO_ELU=1: the consumer applies it while staging)
bool lstm_applies_elu(const Lstm& l);
// Chunk boundaries {0, ..., T} of the layer-pipelined persistent form; {0, T} where the layers run in sequence (fewer than two layers,
// one wanted chunk, a short sequence, or `may_pipe` false).  Host arithmetic only.
std::vector<int64_t> lstm_chunk_starts(int64_t T, int n_layers, int want_chunks, bool even_chunks, bool may_pipe);

// Steps [0, T) of ONE layer in the step-wise form -- the input projections of `in` [N,C,T], then one fresh launch per time step -- from the
// state the caller hands in: h0 and cs are [C][N] (unit-major), h1 is the second half of the double-buffered h.  out [N,C,T] receives h_t
// (+ skip, ELU where asked).  Returns the half (h0 or h1) that holds h_T; cs holds c_T.  Zero state in: SLSTM.forward's own layer.
float* lstm_layer_steps(EncodecModel& m, LstmLayer& y, int C, const float* in, const float* skip, float* out, float* h0, float* h1, float* cs, int N, int64_t T,
                        bool elu_out);

// What a handle's LSTM launches own beside the weights.  It reaches the pool allocator, the stream, the profiler, cu_count, lds_per_cu
// and on_side_group of the model that holds it through `m`.
struct LstmRuntime {
    EncodecModel& m;
    bool force_stepwise = false;   // after a timeout: the persistent form needs its workgroups co-resident, which a busy / partitioned device may not grant
    int64_t timeouts = 0;          // timeouts this handle has seen (nc_encodec_lstm_stats)
    // Timeout word of the persistent kernels: ONE word of pinned, device-mapped host memory -- a kernel that gives up its spin writes it
    // over PCIe, the host reads it without touching the stream.
    unsigned* tmo_host = nullptr;
    unsigned* tmo_dev = nullptr;
    LstmTicket* ticket = nullptr;
    hipStream_t stream2 = nullptr;       // layer-pipelined form: second stream for layer 1 (only the primary segment group pipelines)
    std::vector<hipEvent_t> events;      // and its chunk events

    explicit LstmRuntime(EncodecModel& model) : m(model) {}
    ~LstmRuntime();
    void prepare();                // allocates the timeout word (once; the model's device is current)
    bool timed_out() const { return tmo_host && *reinterpret_cast<volatile unsigned*>(tmo_host) != 0; }
    // Where the word is raised: wait for the model's stream, clear the word, switch the handle to the step-wise kernels (fresh launches
    // need no co-residency) and count it; returns whether it was.
    bool note_timeout();
    // SLSTM.forward (SLSTM.cs:40-57) on a dense x [N,C,T]; returns lstm(x) + x (elu_out: ELU of it)
    float* run(Lstm& l, const float* x, int N, int64_t T, bool elu_out);
};

}  // namespace nc
