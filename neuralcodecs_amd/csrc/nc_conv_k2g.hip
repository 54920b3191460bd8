// Instantiates the sub-pixel transposed convolution for strides that are not a power of two (two taps per phase, SUB == 2).
#include "nc_conv_kernel.hip.h"
NC_INSTANTIATE_CONV(subg_k2, NC_ARGS_TM_TN, TM * 10 + TN, NC_TILES_ALL, 2, 16, 20, false, 2, 4, false, 2)
