// Loudness (include/nc_mi355x.h "loudness"): what the device unit (nc_loudness.hip) and the serial host twin
// (nc_loudness_host.hip) share besides nc_math.h -- the argument checks, the coefficient source and the block-table builder.  Nothing of
// the arithmetic on samples lives here: each unit has its own.
#pragma once
#include <vector>

#include "nc_common.h"

namespace nc {

constexpr int kKwBlock = 64;          // L: samples per filter block (the header states it)
constexpr int kLoudSub = 128;         // samples per first-level sub-block of a cell's energy (the header states it)
constexpr float kGainFactor = 0.11512925464970229f;   // LoudnessMeter.GAIN_FACTOR
constexpr double kGateAbs = 0x1.f791ec6e1d5aap-24;    // the binary64 nearest 10^-6.9309

struct KwTables {
    std::vector<float> Hm, Cm;    // [64][64], [4][64]
    double Gs[kKwBlock][4];
    double M[4][4];
};

struct LoudGeom {
    int N, S;                     // block and step of the gating, in samples
};

// NC_EINVAL unless sample_rate >= 10 and the filter is known
void loudness_check_filter(int sample_rate, int filter);
// the rows of a filter / gain call: pointers, R in [1, 32767], offsets and lengths >= 0
void loudness_check_rows(int R, const int64_t* const* offs, int n_offs, int rows_per_n, const int64_t* n);
// B >= 1, C in [1, 5], B C <= 32767, then the rows (offsets are [B C], lengths [B])
void loudness_check_clips(int B, int C, const int64_t* const* offs, int n_offs, const int64_t* n);
// the checked copy of a loudness call's cfg
nc_loudness_cfg loudness_resolve_cfg(const nc_loudness_cfg* cfg, int sample_rate);
LoudGeom loudness_geom(int sample_rate);

// b[2][3], a[2][3] as the header defines them
void kweight_coeffs(int sample_rate, int filter, double* b, double* a);
void build_kweight_tables(int sample_rate, int filter, KwTables& t);

}  // namespace nc
