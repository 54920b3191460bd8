// Distributed-staging variants of the k = 16 strided convolution and the k = 2 sub-pixel up-convolution (tiny grids, see nc_conv.hip).
#include "nc_conv_kernel.hip.h"
NC_INSTANTIATE_CONV(dist_k16, NC_ARGS_TM_TN, TM * 10 + TN, NC_TILES_DIST, 16, 2, 18, false, 2, 4, true, 0)
NC_INSTANTIATE_CONV(dist_sub_k2, NC_ARGS_TM_TN, TM * 10 + TN, NC_TILES_DIST, 2, 16, 20, false, 2, 4, true, 1)
