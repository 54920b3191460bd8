// Round-trip quality (include/nc_mi355x.h "round-trip quality"): what the device unit (nc_quality.hip) and the serial host
// twin (nc_quality_host.hip) share besides nc_math.h -- the argument checks and the two host table builders.  Nothing of the arithmetic
// on samples lives here: each unit has its own.
#pragma once
#include <vector>

#include "nc_common.h"

namespace nc {

constexpr int kQualityBlock = 128;   // samples per first-level block of the time-domain sums (the header states it)

// NC_EINVAL unless W is a power of two in 32..2048, 1 <= H <= min(W, 512) and the window is known
void quality_check_window(int W, int H, int window);
// the rows of a call: pointers, B in [1, 32767], offsets >= 0, n[b] > W/2 for every W in Ws
void quality_check_rows(int B, const int64_t* const* offs, int n_offs, const int64_t* n, const int* Ws, int n_W);
// the admitted nc_quality_cfg with H = 0 and fmax = 0 resolved
nc_quality_cfg quality_resolve_cfg(const nc_quality_cfg* cfg, int sample_rate);
void quality_check_mel(int sample_rate, int n_mels, float fmin, float fmax);

// C, S [W/2+1][W] as the header defines them
void build_dft_basis(int W, int window, float* C, float* S);
// fb [n_mels][n_fft/2+1], lo / hi [n_mels]; fmax already resolved (> fmin)
void build_mel_filterbank(int sample_rate, int n_mels, int n_fft, float fmin, float fmax, float* fb, int32_t* lo, int32_t* hi);

}  // namespace nc
