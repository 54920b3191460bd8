// Two-input (shortcut + branch) variants of the Encodec input mode: the up-convolutions (two taps per phase; per-phase and sub-pixel forms,
// SEANetDecoder.cs ratios 8 / 5 / 4 / 2).
#include "nc_conv_kernel.hip.h"
NC_INSTANTIATE_CONV(in2_k2, NC_ARGS_TM_TN, TM * 10 + TN, NC_TILES_22, 2, 16, 20, false, 2, 4, false, 0, true)
NC_INSTANTIATE_CONV(in2_sub_k2, NC_ARGS_TM_TN, TM * 10 + TN, NC_TILES_22, 2, 16, 20, false, 2, 4, false, 1, true)
