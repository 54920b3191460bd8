// The two size limits of the convolution template: its tile and sub-pixel row offsets are 32-bit.  launch_conv refuses a layer that
// breaks one of them (NC_EUNSUPPORTED); the long-clip planner (nc_chunk.hip) asks the same questions before anything is launched.
#pragma once
#include <cstdint>

namespace nc {

// every instance: the offsets of a tile of `bm` output rows (+ 4 rows of slack) of pitch y_cstride
inline bool conv_rows_fit32(int bm, int64_t y_cstride, int64_t Tout) { return (int64_t)(bm + 4) * y_cstride + Tout < ((int64_t)1 << 31); }
// multiply-shift sub-pixel form of a transposed conv: all Cout rows of a clip, reaching 3 clips ahead
inline bool conv_subpixel_fits32(int Cout, int64_t y_cstride, int64_t y_bstride, int64_t Tout) {
    return (int64_t)(Cout + 4) * y_cstride + Tout + 3 * y_bstride < ((int64_t)1 << 31);
}

}  // namespace nc
