// Mean of a token row from its sum, for the LayerNorm of the rows-in-registers kernels (linear_rows.h, ff_fused.h, seq_attention.h).
#pragma once
#include "dev.h"

namespace aa {

// 1 / n is a rounded constant, so sum * (1 / n) misses the mean of a CONSTANT row by up to |x| 2^-24 - which a LayerNorm's rstd = eps^-1/2
// turns into 1e-3 of a normalised unit at |x| = 50.  One Newton step (the residual sum - n * mean is exact in an fma) gives the quotient to
// the last bit: the mean of a constant row is that constant, x - mean exactly 0.  On the GPU the empty asm keeps -ffast-math from cancelling
// the step algebraically.
__device__ __forceinline__ float row_mean(float sum, int n) {
    const float inv = 1.0f / (float)n;
    float m = sum * inv;
#if defined(__AMDGCN__)
    asm volatile("" : "+v"(m));
#endif
    return __builtin_fmaf(__builtin_fmaf(-m, (float)n, sum), inv, m);
}

}  // namespace aa
