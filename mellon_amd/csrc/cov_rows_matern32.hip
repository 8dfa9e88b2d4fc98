// k_kernel_matrix_rows for MLN_K_MATERN32 (see cov_rows_impl.h)
#include "cov_rows_impl.h"

MLN_INSTANTIATE_KERNEL_MATRIX_ROWS(MLN_K_MATERN32, false)
