// Classifier-free-guidance mix shared by the two samplers (sample.hip, sample_filter.hip): the value the reference's tensors hold at
// (row, id) -- model-dtype logits, mixed by lm/parallel.py:489-492 `logits * cfg + cfg_logits * (1 - cfg)` as three separately rounded
// tensor ops.  RB = the model dtype is bf16 (every operand and intermediate rounded to bf16).
#pragma once
#include "common.h"

template <bool RB>
__device__ __forceinline__ float cfg_mix(float v, const float* c, float cfg, float one_minus_cfg) {
#pragma clang fp contract(off)
    if (RB) v = (float)(bf16)v;
    if (c) {
        float cv = *c;
        if (RB) cv = (float)(bf16)cv;
        float a = v * cfg;
        float b = cv * one_minus_cfg;
        if (RB) { a = (float)(bf16)a; b = (float)(bf16)b; }
        v = a + b;
        if (RB) v = (float)(bf16)v;
    }
    return v;
}

template <bool RB>
__device__ __forceinline__ float cfg_mixed_value(const float* row, const float* crow, long long i, float cfg, float one_minus_cfg) {
    return cfg_mix<RB>(row[i], crow ? crow + i : nullptr, cfg, one_minus_cfg);
}
