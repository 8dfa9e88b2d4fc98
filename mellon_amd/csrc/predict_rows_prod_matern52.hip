// k_predict_mean_rows_prod for MLN_K_MATERN52 (see predict_rows_impl.h)
#include "predict_rows_impl.h"

MLN_INSTANTIATE_PREDICT_MEAN_ROWS(MLN_K_MATERN52, true)
