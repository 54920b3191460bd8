// Two-input (shortcut + branch) variants of the Encodec input mode: strided down-convolutions k = 10 / 16 (SEANetEncoder.cs ratios 5 / 8).
#include "nc_conv_kernel.hip.h"
NC_INSTANTIATE_CONV(in2_k10, NC_ARGS_TM_TN, TM * 10 + TN, NC_TILES_22, 10, 3, 18, false, 2, 4, false, 0, true)
NC_INSTANTIATE_CONV(in2_k16, NC_ARGS_TM_TN, TM * 10 + TN, NC_TILES_22, 16, 2, 18, false, 2, 4, false, 0, true)
