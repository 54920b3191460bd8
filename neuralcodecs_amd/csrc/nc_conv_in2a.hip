// Two-input (shortcut + branch) variants of the Encodec input mode: strided down-convolutions k = 4 / 8 (SEANetEncoder.cs ratios 2 / 4).
#include "nc_conv_kernel.hip.h"
NC_INSTANTIATE_CONV(in2_k4, NC_ARGS_TM_TN, TM * 10 + TN, NC_TILES_22, 4, 8, 18, false, 2, 4, false, 0, true)
NC_INSTANTIATE_CONV(in2_k8, NC_ARGS_TM_TN, TM * 10 + TN, NC_TILES_22, 8, 4, 18, false, 2, 4, false, 0, true)
