// XV-only instances of the fused residual unit (k = 7 + Snake + 1x1 + skip in one launch; nc_conv_kernel.hip.h "XVK").
#include "nc_conv_kernel.hip.h"
NC_INSTANTIATE_CONV(xv_fused_k7, NC_ARGS_TM, TM * 10 + 2, NC_TILES_XV, 7, 8, 10, true, 2, 4, false, 0, false, true)
