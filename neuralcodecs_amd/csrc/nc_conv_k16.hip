// Instantiates the implicit-GEMM convolution for taps-per-phase K=16 (reduction block of 2 input channels,
// up to 18 prefetched window words per lane).
#include "nc_conv_kernel.hip.h"
NC_INSTANTIATE_CONV_K(16, 2, 18)
NC_INSTANTIATE_CONV(narrow_k16, NC_ARGS_TM, TM * 10 + 1, NC_TILES_TN1, 16, 2, 18, false, 2, 3)
