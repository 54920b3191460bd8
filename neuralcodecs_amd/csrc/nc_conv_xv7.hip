// XV-only instances of the k = 7 residual-unit convolution (nc_conv_kernel.hip.h "XVK"): vectorised one-run staging, legacy modes compiled out.
#include "nc_conv_kernel.hip.h"
NC_INSTANTIATE_CONV(xv_k7, NC_ARGS_TM, TM * 10 + 2, NC_TILES_XV, 7, 8, 10, false, 2, 4, false, 0, false, true)
