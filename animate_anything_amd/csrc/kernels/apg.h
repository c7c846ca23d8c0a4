// Adaptive Projected Guidance (Sadat, Hilliges, Weber, "Eliminating Oversaturation and Artifacts of High Guidance Scales in Diffusion
// Models", 2024; `normalized_guidance` with `project` and the momentum buffer of the paper's pseudo-code, in closed form) on the UNet's
// token-layout output, per clip, as TWO launches without atomics:
//   d   = t - u                                         fp32 (u: unconditional clip, t: text clip)
//   r   = d + beta * r_prev ;  d = r                    only when momentum beta != 0; r is the state the momentum buffer carries
//   dd  = sum d d ,  dt = sum d t ,  tt = sum t t       fp64, over the clip's n = channels * frames * hw elements
//   s   = rho / sqrt(dd)  if rho > 0 and dd > rho^2  else 1
//   p   = s dt / tt       if tt > 0                  else 0
//   a   = 1 + (g - 1)(eta - 1) p ,  c = (g - 1) s       fp64, rounded once to fp32
//   out = a t + c d                                     fp32, rounded once to the storage type, over (or beside) the unconditional half
// Only what the step kernels consume is read or written: frames 1..T of every clip and columns [0, channels), the set of cfg_rescale.h.
// The caller then runs the unchanged step kernel with guidance off.
//  1. apg_moments_kernel  workgroup (part, clip) forms d for APG_ROWS rows of the clip - with momentum: reads r_prev and writes r back
//                         in place, every element by one thread - and reduces d d, d t, t t in fp64 to three partial sums.
//  2. apg_apply_kernel    workgroup (part, clip) adds the clip's partial sums (thread i takes parts i, i + 256, ...; then the same
//                         tree), forms s, p, a, c and writes its own rows.  d comes from the momentum buffer with momentum and is formed
//                         again from t - u without; u is read by the very thread that writes `out` there, so `out` may be the
//                         unconditional half of `tokens` itself.
// Every sum runs in an order the geometry alone fixes: a replay, a second call from the same state and the in-place form repeat the bits
// of an eager out-of-place call.
#pragma once
#include "dev.h"
#include "aa_mi355.h"

namespace aa {

constexpr int APG_THREADS = 256;
constexpr int APG_ROWS = 512;                             // token rows per workgroup, as cfg_rescale.h (128 workgroups per clip at 16 x 64 x 64)
constexpr int APG_LDS_BYTES = 3 * APG_THREADS * 8;        // three fp64 sums per thread

AA_HD inline int apg_parts(const AaApg& p) {
    return (int)(((int64_t)p.frames * p.hw + APG_ROWS - 1) / APG_ROWS);
}

// The workgroup's totals of three per-thread sums, in every thread: through LDS, halving 128, 64, ... 1 (always this order).
__device__ __forceinline__ void apg_block_sum(double& s0, double& s1, double& s2) {
    double* red = reinterpret_cast<double*>(dyn_smem());
    const int tid = (int)threadIdx.x;
    red[tid] = s0;
    red[APG_THREADS + tid] = s1;
    red[2 * APG_THREADS + tid] = s2;
    __syncthreads();
    for (int half = APG_THREADS / 2; half > 0; half >>= 1) {
        if (tid < half) {
            red[tid] += red[tid + half];
            red[APG_THREADS + tid] += red[APG_THREADS + tid + half];
            red[2 * APG_THREADS + tid] += red[2 * APG_THREADS + tid + half];
        }
        __syncthreads();
    }
    s0 = red[0];
    s1 = red[APG_THREADS];
    s2 = red[2 * APG_THREADS];
}

// (rows may be 8 bytes apart - a gathered matrix of conv_out's four columns - so elements are read one by one)
template <typename T>
__global__ void __launch_bounds__(APG_THREADS) apg_moments_kernel(const AaApg p, double* ws) {
    const T* tok = reinterpret_cast<const T*>(p.tokens);
    const int T1 = p.frames + 1;
    const int clip = (int)blockIdx.y, part = (int)blockIdx.x;
    const int rows = p.frames * p.hw;                                             // of this clip, frames 1..T
    const int64_t row_u = ((int64_t)clip * T1 + 1) * p.hw;                        // frame 0 of the UNet output is dropped
    const int64_t row_t = ((int64_t)(p.clips + clip) * T1 + 1) * p.hw;            // [uncond clips | text clips]
    float* mom = p.momentum_buf ? p.momentum_buf + (int64_t)clip * rows * p.channels : nullptr;
    double s_dd = 0.0, s_dt = 0.0, s_tt = 0.0;
    const int end = min(rows, (part + 1) * APG_ROWS);
    for (int r = part * APG_ROWS + (int)threadIdx.x; r < end; r += APG_THREADS) {
        const T* pu = tok + (row_u + r) * p.ld;
        const T* pt = tok + (row_t + r) * p.ld;
        for (int ch = 0; ch < p.channels; ++ch) {
            const float u = (float)pu[ch], t = (float)pt[ch];
            float d = t - u;
            if (mom) {
                float* m = mom + (int64_t)r * p.channels + ch;
                d += p.momentum * *m;
                *m = d;
            }
            const double dd = (double)d, td = (double)t;
            s_dd += dd * dd;
            s_dt += dd * td;
            s_tt += td * td;
        }
    }
    apg_block_sum(s_dd, s_dt, s_tt);
    if (threadIdx.x == 0) {
        double* o = ws + ((int64_t)clip * gridDim.x + part) * 3;
        o[0] = s_dd;
        o[1] = s_dt;
        o[2] = s_tt;
    }
}

template <typename T>
__global__ void __launch_bounds__(APG_THREADS) apg_apply_kernel(const AaApg p, const double* ws) {
    const T* tok = reinterpret_cast<const T*>(p.tokens);
    T* out = reinterpret_cast<T*>(p.out);
    const int T1 = p.frames + 1;
    const int clip = (int)blockIdx.y, part = (int)blockIdx.x, parts = (int)gridDim.x;
    const int rows = p.frames * p.hw;
    double s_dd = 0.0, s_dt = 0.0, s_tt = 0.0;
    for (int q = (int)threadIdx.x; q < parts; q += APG_THREADS) {
        const double* w = ws + ((int64_t)clip * parts + q) * 3;
        s_dd += w[0];
        s_dt += w[1];
        s_tt += w[2];
    }
    apg_block_sum(s_dd, s_dt, s_tt);
    const double rho = (double)p.norm_threshold, g1 = (double)p.guidance - 1.0;
    double s = 1.0, par = 0.0;
    if (rho > 0.0 && s_dd > rho * rho) s = rho / sqrt(s_dd);
    if (s_tt > 0.0) par = s * s_dt / s_tt;                                        // (a text clip of zeros has no direction)
    const float a = (float)(1.0 + g1 * ((double)p.eta - 1.0) * par), c = (float)(g1 * s);
    if (p.stats && part == 0 && threadIdx.x == 0) {
        p.stats[2 * clip] = (float)s;
        p.stats[2 * clip + 1] = (float)par;
    }
    const int64_t row_u = ((int64_t)clip * T1 + 1) * p.hw;
    const int64_t row_t = ((int64_t)(p.clips + clip) * T1 + 1) * p.hw;
    const float* mom = p.momentum_buf ? p.momentum_buf + (int64_t)clip * rows * p.channels : nullptr;
    const int end = min(rows, (part + 1) * APG_ROWS);
    for (int r = part * APG_ROWS + (int)threadIdx.x; r < end; r += APG_THREADS) {
        const T* pu = tok + (row_u + r) * p.ld;
        const T* pt = tok + (row_t + r) * p.ld;
        T* po = out + (row_u + r) * p.out_ld;
        for (int ch = 0; ch < p.channels; ++ch) {
            const float t = (float)pt[ch];
            const float d = mom ? mom[(int64_t)r * p.channels + ch] : t - (float)pu[ch];
            po[ch] = (T)(a * t + c * d);                                          // the one rounding to the storage type
        }
    }
}

}  // namespace aa
