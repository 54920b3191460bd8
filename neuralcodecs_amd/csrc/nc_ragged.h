// The table-driven copies of the ragged batch calls (nc_ragged.hip), shared by the codecs' ragged drivers.
// A descriptor is a run of n elements from src to dst followed by `fill` zeros.  Every descriptor of every launch of a call is written
// (and bounds-checked against the tensors it addresses) before anything is launched; rg_upload() then makes one pinned image and one
// asynchronous copy of them on the handle's stream.
#pragma once
#include <algorithm>
#include <vector>

#include "nc_model.h"

namespace nc {

constexpr int32_t kRaggedDefaultMaxWindows = 128;   // rows per launch batch where the handle sets none

struct RgSeg { int64_t src, dst, n, fill; };   // elements

struct RgTables {
    struct Launch { size_t first, count; int64_t longest; };
    std::vector<RgSeg> segs;
    std::vector<Launch> launches;
    std::vector<char> extra;   // further tables of the call (multiples of 8 bytes), placed behind the descriptors in the same image
    size_t open_at = 0;
    int64_t src_elems = 0, dst_elems = 0, longest = 0;

    void begin(int64_t src_n, int64_t dst_n) { open_at = segs.size(); src_elems = src_n; dst_elems = dst_n; longest = 0; }
    void add(int64_t src, int64_t dst, int64_t n, int64_t fill = 0) {
        if (n < 0 || fill < 0 || src < 0 || dst < 0 || src + n > src_elems || dst + n + fill > dst_elems)
            fail(NC_ESTATE, "internal: ragged descriptor [%lld + %lld] -> [%lld + %lld] leaves its tensors (%lld, %lld elements)", (long long)src,
                 (long long)n, (long long)dst, (long long)(n + fill), (long long)src_elems, (long long)dst_elems);
        if (n + fill == 0) return;
        segs.push_back({src, dst, n, fill});
        longest = std::max(longest, n + fill);
    }
    size_t end() {   // -> index of the launch
        launches.push_back({open_at, segs.size() - open_at, longest});
        return launches.size() - 1;
    }
};

// one pinned image, one asynchronous copy on m.stream; returns the device address of `extra` (null when it is empty)
const char* rg_upload(Codec& m, const RgTables& t);
// launch `which` of the uploaded tables on m.stream: 16-byte stores on the destination side, any alignment on the source
void rg_copy_f32(Codec& m, const RgTables& t, size_t which, const float* src, float* dst);
void rg_copy_i64(Codec& m, const RgTables& t, size_t which, const int64_t* src, int64_t* dst);

}  // namespace nc
