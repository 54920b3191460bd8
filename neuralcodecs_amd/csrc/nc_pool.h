// The small parts every slot pool and table-driven driver on the host is made of (nc_session_pool.hip, nc_encodec_stream.hip,
// nc_encodec_causal.hip; the launch loops of nc_ragged.hip and nc_encodec_ragged.hip too).  Parts, not a pool type: each pool keeps its
// own planner, geometry and step.
#pragma once
#include <algorithm>
#include <vector>

#include "nc_model.h"

namespace nc {

constexpr int64_t kAlign = 64;   // elements: every batch tensor of an arena starts on a 256-byte (float) boundary, as an allocation of its own would
inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

// a packed host tensor to its staging buffer, on the stream
inline void h2d(DevBuf& d, const void* h, size_t n, hipStream_t s) {
    d.reserve(std::max<size_t>(n, 16));
    if (n) NC_HIP(hipMemcpyAsync(d.p, h, n, hipMemcpyHostToDevice, s));
}

// grid.y holds 65535 descriptors: fn(first, count) for every run of at most that many out of n
template <class F>
void for_grid_y(size_t n, F&& fn) {
    for (size_t done = 0; done < n; done += 65535) fn(done, std::min<size_t>(65535, n - done));
}

// A carry of [2][n_slots][cap] elements: a slot's state is in the half its `cur` names, a step writes the other half and flips the
// slot, so no launch reads what it writes.
struct TwoHalves {
    int64_t n_slots = 0, cap = 0;
    int64_t at(int half, int slot) const { return ((int64_t)half * n_slots + slot) * cap; }
    int64_t elems() const { return 2 * n_slots * cap; }
};
// A slot starts over in the half it is in: work already queued may still read this half; a new stream reads neither before it has
// written one (and starts from zero state).
template <class S>
void reset_keep_cur(S& s) {
    const int cur = s.cur;
    s = S{};
    s.cur = cur;
}

// The pool behind an opaque handle; the slot of an index.  The wording is the pool's own: Pool::kNull, and Pool::kRange with the slot
// and Pool::kRangeLast (0: the number of slots, 1: the last slot) as its arguments.
template <class Pool>
Pool& pool_of(const Pool* p) {
    if (!p) fail(NC_EINVAL, "%s", Pool::kNull);
    return *const_cast<Pool*>(p);
}
template <class Pool>
typename Pool::Slot& slot_of(Pool& p, int32_t slot) {
    if (slot < 0 || slot >= p.n_slots()) fail(NC_EINVAL, Pool::kRange, slot, (long long)p.n_slots() - Pool::kRangeLast);
    return p.slots[(size_t)slot];
}
constexpr const char* kSlotOutOfRange = "slot %d is out of range (the pool has %lld)";   // the Encodec pools

// ---- the two Encodec pools ---------------------------------------------------------------------------------------------------------
// Every refusal of a step that needs the slots' state alone; T0 and `second` (the slot's other counter) of the named slots come back.
template <class Pool>
void pool_named_slots(const Pool& x, int n, const int32_t* ids, const int64_t* n_in, const char* what, int64_t Pool::Slot::*second_of,
                      std::vector<int64_t>& T0, std::vector<int64_t>& second) {
    if (!ids || !n_in) fail(NC_EINVAL, "%s: null pointer", what);
    if (n <= 0) fail(NC_EINVAL, "%s: n must be positive", what);
    std::vector<char> seen(x.slots.size(), 0);
    T0.resize((size_t)n); second.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (ids[i] < 0 || ids[i] >= x.n_slots()) fail(NC_EINVAL, "%s: slot %d is out of range (the pool has %lld)", what, ids[i], (long long)x.n_slots());
        if (seen[(size_t)ids[i]]) fail(NC_EINVAL, "%s: slot %d is named twice", what, ids[i]);
        seen[(size_t)ids[i]] = 1;
        const typename Pool::Slot& s = x.slots[(size_t)ids[i]];
        if (s.ended) fail(NC_EINVAL, "%s: slot %d has been flushed: reset it before the next stream", what, ids[i]);
        T0[(size_t)i] = s.T; second[(size_t)i] = s.*second_of;
    }
}

// A host-pointer step: `in` staged in, run(in, out, emb) on the staged tensors, `out` and the embeddings copied back, complete on return.
// The pool owns in_stage, out_stage and emb_stage.  Sizes in bytes.
template <class Pool, class Run>
void pool_step_staged(Pool& x, hipStream_t s, const void* in, size_t in_bytes, void* out, size_t out_bytes, float* emb, size_t emb_bytes, Run&& run) {
    h2d(x.in_stage, in, in_bytes, s);
    x.out_stage.reserve(std::max<size_t>(out_bytes, 16));
    if (emb) x.emb_stage.reserve(std::max<size_t>(emb_bytes, 16));
    run(x.in_stage.p, x.out_stage.p, emb ? x.emb_stage.template as<float>() : nullptr);
    if (out_bytes) NC_HIP(hipMemcpyAsync(out, x.out_stage.p, out_bytes, hipMemcpyDeviceToHost, s));
    if (emb && emb_bytes) NC_HIP(hipMemcpyAsync(emb, x.emb_stage.p, emb_bytes, hipMemcpyDeviceToHost, s));
    NC_HIP(hipStreamSynchronize(s));
}

}  // namespace nc
