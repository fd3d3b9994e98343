// The one function of head.hip that another translation unit calls: norm.hip's gdl_bn_head_bwd_reduce writes the head's
// weight-gradient partial rows itself and hands them to the head's final reduction.
#pragma once
#include "gdl_common.h"

// ws[nsplit][K + 1][C] partial rows -> dw [K][C], db [K] (db may be null); GDL_ERR_UNSUPPORTED for K outside 1..16
int head_bwd_w_final_launch(const float* ws, int nsplit, int C, int K, float* dw, float* db, hipStream_t s);
