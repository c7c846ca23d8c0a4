// guidance_rescale (Lin et al., "Common Diffusion Noise Schedules and Sample Steps are Flawed", section 3.4; diffusers `rescale_noise_cfg`)
// on the UNet's token-layout output, per clip, as TWO launches without atomics:
//   c = u + g * (t - u)                              fp32, the expression of guided_token() (glue.h)
//   k_b = 1 + phi * (std(t) / std(c) - 1)            unbiased deviations over the clip's n = channels * frames * hw elements
//   out = k_b * c                                    rounded once to the storage type, written over (or beside) the unconditional half
// Only what the step kernels consume is read or written: frames 1..T of every clip (rows [(b * (T+1) + 1) * hw, (b + 1) * (T+1) * hw) of
// the matrix, one contiguous run per clip) and columns [0, channels).  The caller then runs the unchanged step kernel with guidance off.
//  1. cfg_rescale_moments_kernel  workgroup (part, clip) reduces CR_ROWS rows of the clip to the sums of dt, dt^2, dc, dc^2 in fp64, with
//                                 dt = t - t_0 and dc = c - c_0 taken against the clip's FIRST element: the variance does not depend on the
//                                 shift, inputs of mean 50 lose nothing to the cancellation, and a constant clip sums exact zeros.
//  2. cfg_rescale_apply_kernel    workgroup (part, clip) adds the clip's partial sums (thread i takes parts i, i + 256, ...; then the same
//                                 tree), forms k_b and scales its own rows; every element is read and written by one thread, so `out` may
//                                 be the unconditional half of `tokens` itself.
// Every sum runs in an order the geometry alone fixes: a replay, a second call and the in-place form repeat the bits of an eager call.
// DEPARTURE from diffusers: a clip whose guided prediction is constant (std(c) == 0) makes diffusers divide by zero (NaN); here k_b = 1
// and the prediction is left unscaled.
#pragma once
#include "dev.h"
#include "aa_mi355.h"

namespace aa {

constexpr int CR_THREADS = 256;
constexpr int CR_ROWS = 512;                              // token rows per workgroup: two per thread (128 workgroups per clip at 16 x 64 x 64)
constexpr int CR_LDS_BYTES = 4 * CR_THREADS * 8;          // four fp64 sums per thread

AA_HD inline int cr_parts(const AaCfgRescale& p) {
    return (int)(((int64_t)p.frames * p.hw + CR_ROWS - 1) / CR_ROWS);
}

// The workgroup's totals of four per-thread sums, in every thread: through LDS, halving 128, 64, ... 1 (always this order).
__device__ __forceinline__ void cr_block_sum(double& s0, double& s1, double& s2, double& s3) {
    double* red = reinterpret_cast<double*>(dyn_smem());
    const int tid = (int)threadIdx.x;
    red[tid] = s0;
    red[CR_THREADS + tid] = s1;
    red[2 * CR_THREADS + tid] = s2;
    red[3 * CR_THREADS + tid] = s3;
    __syncthreads();
    for (int half = CR_THREADS / 2; half > 0; half >>= 1) {
        if (tid < half) {
            red[tid] += red[tid + half];
            red[CR_THREADS + tid] += red[CR_THREADS + tid + half];
            red[2 * CR_THREADS + tid] += red[2 * CR_THREADS + tid + half];
            red[3 * CR_THREADS + tid] += red[3 * CR_THREADS + tid + half];
        }
        __syncthreads();
    }
    s0 = red[0];
    s1 = red[CR_THREADS];
    s2 = red[2 * CR_THREADS];
    s3 = red[3 * CR_THREADS];
}

// (rows may be 8 bytes apart - a gathered matrix of conv_out's four columns - so elements are read one by one)
template <typename T>
__global__ void __launch_bounds__(CR_THREADS) cfg_rescale_moments_kernel(const AaCfgRescale p, double* ws) {
    const T* tok = reinterpret_cast<const T*>(p.tokens);
    const int T1 = p.frames + 1;
    const int clip = (int)blockIdx.y, part = (int)blockIdx.x;
    const int rows = p.frames * p.hw;                                             // of this clip, frames 1..T
    const int64_t row_u = ((int64_t)clip * T1 + 1) * p.hw;                        // frame 0 of the UNet output is dropped
    const int64_t row_t = ((int64_t)(p.clips + clip) * T1 + 1) * p.hw;            // [uncond clips | text clips]
    const float u0 = (float)tok[row_u * p.ld], t0 = (float)tok[row_t * p.ld];
    const double sh_t = (double)t0, sh_c = (double)(u0 + p.guidance * (t0 - u0));
    double s_t = 0.0, s_tt = 0.0, s_c = 0.0, s_cc = 0.0;
    const int end = min(rows, (part + 1) * CR_ROWS);
    for (int r = part * CR_ROWS + (int)threadIdx.x; r < end; r += CR_THREADS) {
        const T* pu = tok + (row_u + r) * p.ld;
        const T* pt = tok + (row_t + r) * p.ld;
        for (int ch = 0; ch < p.channels; ++ch) {
            const float u = (float)pu[ch], t = (float)pt[ch];
            const float c = u + p.guidance * (t - u);
            const double dt = (double)t - sh_t, dc = (double)c - sh_c;
            s_t += dt;
            s_tt += dt * dt;
            s_c += dc;
            s_cc += dc * dc;
        }
    }
    cr_block_sum(s_t, s_tt, s_c, s_cc);
    if (threadIdx.x == 0) {
        double* o = ws + ((int64_t)clip * gridDim.x + part) * 4;
        o[0] = s_t;
        o[1] = s_tt;
        o[2] = s_c;
        o[3] = s_cc;
    }
}

template <typename T>
__global__ void __launch_bounds__(CR_THREADS) cfg_rescale_apply_kernel(const AaCfgRescale p, const double* ws) {
    const T* tok = reinterpret_cast<const T*>(p.tokens);
    T* out = reinterpret_cast<T*>(p.out);
    const int T1 = p.frames + 1;
    const int clip = (int)blockIdx.y, part = (int)blockIdx.x, parts = (int)gridDim.x;
    const int rows = p.frames * p.hw;
    double s_t = 0.0, s_tt = 0.0, s_c = 0.0, s_cc = 0.0;
    for (int q = (int)threadIdx.x; q < parts; q += CR_THREADS) {
        const double* w = ws + ((int64_t)clip * parts + q) * 4;
        s_t += w[0];
        s_tt += w[1];
        s_c += w[2];
        s_cc += w[3];
    }
    cr_block_sum(s_t, s_tt, s_c, s_cc);
    // (n - 1) * variance; the common 1 / (n - 1) drops out of the ratio
    const double n = (double)rows * (double)p.channels;
    const double q_t = s_tt - s_t * s_t / n, q_c = s_cc - s_c * s_c / n;
    float k = 1.0f;
    if (p.rescale != 0.0f && q_c > 0.0) k = (float)(1.0 + (double)p.rescale * (sqrt(fmax(q_t, 0.0) / q_c) - 1.0));
    if (p.factor && part == 0 && threadIdx.x == 0) p.factor[clip] = k;
    const int64_t row_u = ((int64_t)clip * T1 + 1) * p.hw;
    const int64_t row_t = ((int64_t)(p.clips + clip) * T1 + 1) * p.hw;
    const int end = min(rows, (part + 1) * CR_ROWS);
    for (int r = part * CR_ROWS + (int)threadIdx.x; r < end; r += CR_THREADS) {
        const T* pu = tok + (row_u + r) * p.ld;
        const T* pt = tok + (row_t + r) * p.ld;
        T* po = out + (row_u + r) * p.out_ld;
        for (int ch = 0; ch < p.channels; ++ch) {
            const float u = (float)pu[ch], t = (float)pt[ch];
            const float c = u + p.guidance * (t - u);
            po[ch] = (T)(k * c);                                                  // the one rounding to the storage type
        }
    }
}

}  // namespace aa
