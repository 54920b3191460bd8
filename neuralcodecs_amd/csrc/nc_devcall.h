// The host scaffold of the signal tools that are tied to a device, not to a codec handle (nc_quality.hip, nc_loudness.hip, nc_resample.hip;
// DESIGN.md 4p).  A unit keeps ONE State per device behind ONE lock of its own; State holds a DevCall next to
// the unit's caches and workspace.  The cross-stream rule lives here and nowhere else: a call on another stream first waits for the call
// before it (`done`), and the pinned image is written again only after the previous call's copy has read it (`copied`).
#pragma once
#include <map>
#include <mutex>

#include "nc_common.h"

namespace nc {

struct DevCall {
    DevBuf tables;   // the device copy of the call's row tables
    void* pin = nullptr;
    size_t pin_cap = 0;
    hipEvent_t copied = nullptr, done = nullptr;
    bool copied_used = false, done_used = false;

    void begin(hipStream_t s) {
        if (!copied) NC_HIP(hipEventCreateWithFlags(&copied, hipEventDisableTiming));
        if (!done) NC_HIP(hipEventCreateWithFlags(&done, hipEventDisableTiming));
        if (done_used) NC_HIP(hipStreamWaitEvent(s, done, 0));
    }
    void end(hipStream_t s) {
        NC_HIP(hipGetLastError());
        NC_HIP(hipEventRecord(done, s));
        done_used = true;
    }
    // the row tables of a call: written into pinned memory, copied once
    void* upload(const void* src, size_t bytes, hipStream_t s) {
        if (copied_used) NC_HIP(hipEventSynchronize(copied));   // the previous call's copy has read the pinned image
        if (bytes > pin_cap) {
            if (pin) (void)hipHostFree(pin);
            pin = nullptr;
            pin_cap = 0;
            const size_t want = (bytes + 4095) & ~size_t(4095);
            NC_HIP(hipHostMalloc(&pin, want, hipHostMallocDefault));
            pin_cap = want;
        }
        memcpy(pin, src, bytes);
        tables.reserve(bytes);
        NC_HIP(hipMemcpyAsync(tables.p, pin, bytes, hipMemcpyHostToDevice, s));
        NC_HIP(hipEventRecord(copied, s));
        copied_used = true;
        return tables.p;
    }
    template <class T>
    const T* upload(const std::vector<T>& rows, hipStream_t s) { return static_cast<const T*>(upload(rows.data(), rows.size() * sizeof(T), s)); }
};

// One State per device behind the unit's own lock.  An entry point validates its arguments first, then: switch device, take the lock, run.
template <class State>
struct PerDevice {
    std::mutex mu;
    // never destroyed: the buffers must not be freed behind the runtime's own teardown at process exit
    std::map<int, State>& dev = *new std::map<int, State>();
    template <class F>
    void locked(int device_index, F&& f) {
        use_checked_device(device_index);
        std::lock_guard<std::mutex> lk(mu);
        f(dev[device_index]);
    }
};

// A table built on the host on first use and cached in the unit's map: build(fresh) fills a fresh Slot with blocking copies (fill_table)
// under the unit's lock, so the table has arrived before this or any later call, on whichever stream, launches a kernel that reads it.
// The slot is published only after the last copy has returned: a failed upload leaves it empty and the next call builds it again.
inline bool filled(const DevBuf& d) { return d.p != nullptr; }
template <class Slot, class Build>
const Slot& cached_table(Slot& slot, Build&& build) {
    if (!filled(slot)) {
        Slot fresh;
        build(fresh);
        slot = std::move(fresh);
    }
    return slot;
}
template <class T>
void fill_table(DevBuf& d, const T* h, size_t count) {
    d.reserve(count * sizeof(T));
    NC_HIP(hipMemcpy(d.p, h, count * sizeof(T), hipMemcpyHostToDevice));
}

// The float rows of a HOST-buffer call packed end to end for the device: row r has len[r / rows_per_len] elements and starts at element
// at[r], a multiple of `align`.  copy_in / copy_out are blocking, one hipMemcpy per non-empty row; the call between them runs on the
// null stream and the caller synchronises it.
struct PackedRows {
    std::vector<int64_t> at;
    int64_t total = 0;
    const int64_t* len;
    int rows_per_len;
    PackedRows(int R, const int64_t* len_, int rows_per_len_, int64_t align) : at((size_t)R), len(len_), rows_per_len(rows_per_len_) {
        for (int r = 0; r < R; ++r) {
            at[(size_t)r] = total;
            total += (n(r) + align - 1) / align * align;
        }
    }
    int64_t n(int r) const { return len[r / rows_per_len]; }
    void reserve(DevBuf& d) const { d.reserve((size_t)(total > 0 ? total : 1) * sizeof(float)); }
    void copy_in(DevBuf& d, const float* src, const int64_t* off) const {
        reserve(d);
        for (int r = 0; r < (int)at.size(); ++r)
            if (n(r) > 0) NC_HIP(hipMemcpy(d.as<float>() + at[(size_t)r], src + off[r], (size_t)n(r) * sizeof(float), hipMemcpyHostToDevice));
    }
    void copy_out(const DevBuf& d, float* dst, const int64_t* off) const {
        for (int r = 0; r < (int)at.size(); ++r)
            if (n(r) > 0) NC_HIP(hipMemcpy(dst + off[r], d.as<float>() + at[(size_t)r], (size_t)n(r) * sizeof(float), hipMemcpyDeviceToHost));
    }
};

// blocks of per_block items; the unit names its own limit
inline unsigned grid_of(int64_t items, int per_block, int64_t max_blocks) {
    const int64_t g = (items + per_block - 1) / per_block;
    if (g > max_blocks) fail(NC_EINVAL, "a row is too long for one launch");
    return (unsigned)(g > 0 ? g : 1);
}

}  // namespace nc
