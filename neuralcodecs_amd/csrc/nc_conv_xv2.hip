// XV-only instances of the two-tap sub-pixel up-convolutions (power-of-two strides; nc_conv_kernel.hip.h "XVK").
#include "nc_conv_kernel.hip.h"
NC_INSTANTIATE_CONV(xv_sub_k2, NC_ARGS_TM, TM * 10 + 2, NC_TILES_XV, 2, 16, 20, false, 2, 4, false, 1, false, true)
