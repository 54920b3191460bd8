// Instantiates the implicit-GEMM convolution for taps-per-phase K=3 (reduction block of 16 input channels,
// up to 20 prefetched window words per lane).
#include "nc_conv_kernel.hip.h"
NC_INSTANTIATE_CONV_K(3, 16, 20)
NC_INSTANTIATE_CONV(narrow_k3, NC_ARGS_TM, TM * 10 + 1, NC_TILES_TN1, 3, 16, 20, false, 2, 3)
NC_INSTANTIATE_CONV(slim_k3, NC_ARGS_TM_TN, TM * 10 + TN, NC_TILES_22, 3, 8, 10, false, 4)
