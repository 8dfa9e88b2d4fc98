// k_kernel_matrix_rows_prod for MLN_K_MATERN32 (see kernel_rows_prod_impl.h)
#include "kernel_rows_prod_impl.h"

MLN_DEFINE_ROWS_PROD_KIND(MLN_K_MATERN32)
