// Instantiates the implicit-GEMM convolution for taps-per-phase K=7 (reduction block of 8 input channels,
// up to 10 prefetched window words per lane).
#include "nc_conv_kernel.hip.h"
NC_INSTANTIATE_CONV_K(7, 8, 10)

NC_INSTANTIATE_CONV(narrow_k7, NC_ARGS_TM, TM * 10 + 1, NC_TILES_TN1, 7, 8, 10, false, 2, 3)
NC_INSTANTIATE_CONV(slim_k7, NC_ARGS_TM_TN, TM * 10 + TN, NC_TILES_22, 7, 4, 5, false, 4)
