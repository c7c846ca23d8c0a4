// FreeInit (Wu et al., "FreeInit: Bridging Initialization Gap in Video Diffusion Models"; diffusers `FreeInitMixin`) re-initialisation
// of the latents between two sampling iterations, per (clip, channel) volume of contiguous fp32 [frames][h][w]:
//     out = z + LP(a * x + s * n0 - z)          LP(d) = Re IFFT3(Ms * FFT3 d)
// x: the previous iteration's result, n0: the run's initial noise, z: fresh noise, Ms: the low-pass mask in UNSHIFTED order, symmetrised
// (Ms[k] = (Mu[k] + Mu[-k]) / 2: a real operator, so no complex output exists - DESIGN.md section 13).  No FFT: every axis is 1 .. 128 long
// and need not be a power of two, so each axis is a direct DFT from a host-built (cos, sin) table of n entries indexed by j * k mod n
// (kept as a running index: no multiplication, no division in the sum).  Five launches over one complex workspace [volumes][frames][h][w]:
//  1. freeinit_rows_fwd_kernel    d = (a x + s n0) - z formed on the way in, real-to-complex DFT along w
//  2. freeinit_axis_kernel<false> DFT along h, in place
//  3. freeinit_frames_kernel      DFT along frames, times Ms / (frames h w), inverse DFT along frames, in place (the line stays in LDS)
//  4. freeinit_axis_kernel<true>  inverse DFT along h, in place
//  5. freeinit_rows_inv_kernel    the real part of the inverse DFT along w, plus z, stored
// A workgroup stages the lines it owns in LDS next to the axis' table, meets a barrier and only then writes: in place is safe, and
// `out` may be `x` (read by launch 1 alone).  On the strided axes a workgroup owns FI_XB ADJACENT lines, so global accesses run along
// the contiguous axis (128-byte runs) and the LDS reads of a wave are FI_XB consecutive 8-byte words (no bank conflict) plus at most
// four table entries.  Every sum runs j = 0 .. n-1 in one thread: no atomics, no cross-lane reduction; a replay repeats the bits.
#pragma once
#include "dev.h"
#include "aa_mi355.h"

namespace aa {

constexpr int FI_THREADS = 256;
constexpr int FI_MAX = 128;                                // longest axis
constexpr int FI_XB = 16;                                  // adjacent lines per workgroup on the strided axes
constexpr int FI_ROW_TILE = 1024;                          // elements per workgroup on the w axis (whole rows: at least 8 of them)
constexpr int FI_TW_BYTES = FI_MAX * 8;
constexpr int FI_ROWS_FWD_LDS = FI_TW_BYTES + FI_ROW_TILE * 4;
constexpr int FI_ROWS_INV_LDS = FI_TW_BYTES + FI_ROW_TILE * 8;
constexpr int FI_AXIS_LDS = FI_TW_BYTES + FI_MAX * FI_XB * 8;
constexpr int FI_FRAMES_LDS = FI_TW_BYTES + 2 * FI_MAX * FI_XB * 8;

AA_HD inline int fi_rows_per_group(int w) { return FI_ROW_TILE / w; }
AA_HD inline int64_t fi_row_groups(const AaFreeInit& p) {
    const int64_t rows = (int64_t)p.volumes * p.frames * p.h;
    const int r = fi_rows_per_group(p.w);
    return (rows + r - 1) / r;
}
AA_HD inline int64_t fi_axis_groups(int64_t outer, int64_t inner) { return outer * ((inner + FI_XB - 1) / FI_XB); }
// the (cos, sin) tables of the three axes in one array: [frames] entries, then [h], then [w]
AA_HD inline int fi_tw_frames(const AaFreeInit&) { return 0; }
AA_HD inline int fi_tw_h(const AaFreeInit& p) { return p.frames; }
AA_HD inline int fi_tw_w(const AaFreeInit& p) { return p.frames + p.h; }

__device__ __forceinline__ f32x2* fi_stage_table(const f32x2* table, int n) {
    f32x2* tw = reinterpret_cast<f32x2*>(dyn_smem());
    for (int i = (int)threadIdx.x; i < n; i += FI_THREADS) tw[i] = table[i];
    return tw;
}

// v * e^(-i theta) (forward) or v * e^(+i theta) (inverse) added to (re, im); t = (cos theta, sin theta)
template <bool INV>
__device__ __forceinline__ void fi_cmac(float& re, float& im, const f32x2 v, const f32x2 t) {
    if constexpr (INV) {
        re += v[0] * t[0];
        re -= v[1] * t[1];
        im += v[0] * t[1];
        im += v[1] * t[0];
    } else {
        re += v[0] * t[0];
        re += v[1] * t[1];
        im += v[1] * t[0];
        im -= v[0] * t[1];
    }
}

// 1. grid: fi_row_groups.  Workgroup g owns rows [g R, (g + 1) R) of the [volumes * frames * h] rows of w elements.
template <int UNIT = 0>          // (a template only so that the header may be included by several translation units)
__global__ void __launch_bounds__(FI_THREADS) freeinit_rows_fwd_kernel(const AaFreeInit p, f32x2* ws) {
    const int w = p.w, R = fi_rows_per_group(w);
    const int64_t rows = (int64_t)p.volumes * p.frames * p.h;
    const int64_t row0 = (int64_t)blockIdx.x * R;
    const int count = (int)(rows - row0 < R ? rows - row0 : R) * w;
    const int64_t base = row0 * w;
    const f32x2* tw = fi_stage_table(reinterpret_cast<const f32x2*>(p.twiddle) + fi_tw_w(p), w);
    float* tile = reinterpret_cast<float*>(dyn_smem() + FI_TW_BYTES);
    for (int i = (int)threadIdx.x; i < count; i += FI_THREADS)
        tile[i] = (p.a * p.x[base + i] + p.s * p.n0[base + i]) - p.z[base + i];
    __syncthreads();
    for (int o = (int)threadIdx.x; o < count; o += FI_THREADS) {
        const int r = o / w, k = o - r * w;
        const float* line = tile + r * w;
        float re = 0.0f, im = 0.0f;
        int idx = 0;
        for (int j = 0; j < w; ++j) {
            const f32x2 t = tw[idx];
            re += line[j] * t[0];
            im -= line[j] * t[1];
            idx += k;
            if (idx >= w) idx -= w;
        }
        ws[base + o] = f32x2{re, im};
    }
}

// 2. / 4. grid: fi_axis_groups(outer, inner).  The array is [outer][n][inner]; a workgroup owns the lines (o, *, x0 .. x0 + FI_XB).
template <bool INV>
__global__ void __launch_bounds__(FI_THREADS) freeinit_axis_kernel(f32x2* ws, const f32x2* table, int n, int inner) {
    const int chunks = (inner + FI_XB - 1) / FI_XB;
    const int64_t o_idx = (int64_t)blockIdx.x / chunks;
    const int x0 = (int)((int64_t)blockIdx.x - o_idx * chunks) * FI_XB;
    f32x2* g = ws + o_idx * n * inner + x0;
    const f32x2* tw = fi_stage_table(table, n);
    f32x2* tile = reinterpret_cast<f32x2*>(dyn_smem() + FI_TW_BYTES);
    const int count = n * FI_XB;
    for (int i = (int)threadIdx.x; i < count; i += FI_THREADS) {
        const int j = i / FI_XB, xl = i % FI_XB;
        tile[i] = x0 + xl < inner ? g[(int64_t)j * inner + xl] : f32x2{0.0f, 0.0f};
    }
    __syncthreads();
    for (int o = (int)threadIdx.x; o < count; o += FI_THREADS) {
        const int k = o / FI_XB, xl = o % FI_XB;
        float re = 0.0f, im = 0.0f;
        int idx = 0;
        for (int j = 0; j < n; ++j) {
            fi_cmac<INV>(re, im, tile[j * FI_XB + xl], tw[idx]);
            idx += k;
            if (idx >= n) idx -= n;
        }
        if (x0 + xl < inner) g[(int64_t)k * inner + xl] = f32x2{re, im};
    }
}

// 3. grid: fi_axis_groups(volumes, h * w).  The array is [volumes][frames][h * w]; forward along frames, the mask, inverse along frames.
template <int UNIT = 0>          // (a template only so that the header may be included by several translation units)
__global__ void __launch_bounds__(FI_THREADS) freeinit_frames_kernel(const AaFreeInit p, f32x2* ws) {
    const int n = p.frames, inner = p.h * p.w;
    const int chunks = (inner + FI_XB - 1) / FI_XB;
    const int64_t vol = (int64_t)blockIdx.x / chunks;
    const int x0 = (int)((int64_t)blockIdx.x - vol * chunks) * FI_XB;
    f32x2* g = ws + vol * n * inner + x0;
    const float* mask = p.mask + x0;
    const f32x2* tw = fi_stage_table(reinterpret_cast<const f32x2*>(p.twiddle) + fi_tw_frames(p), n);
    f32x2* tile = reinterpret_cast<f32x2*>(dyn_smem() + FI_TW_BYTES);
    f32x2* spec = tile + FI_MAX * FI_XB;
    const float scale = 1.0f / ((float)n * (float)inner);
    const int count = n * FI_XB;
    for (int i = (int)threadIdx.x; i < count; i += FI_THREADS) {
        const int j = i / FI_XB, xl = i % FI_XB;
        tile[i] = x0 + xl < inner ? g[(int64_t)j * inner + xl] : f32x2{0.0f, 0.0f};
    }
    __syncthreads();
    for (int o = (int)threadIdx.x; o < count; o += FI_THREADS) {
        const int k = o / FI_XB, xl = o % FI_XB;
        float re = 0.0f, im = 0.0f;
        int idx = 0;
        for (int j = 0; j < n; ++j) {
            fi_cmac<false>(re, im, tile[j * FI_XB + xl], tw[idx]);
            idx += k;
            if (idx >= n) idx -= n;
        }
        const float m = x0 + xl < inner ? mask[(int64_t)k * inner + xl] * scale : 0.0f;
        spec[o] = f32x2{re * m, im * m};
    }
    __syncthreads();
    for (int o = (int)threadIdx.x; o < count; o += FI_THREADS) {
        const int k = o / FI_XB, xl = o % FI_XB;
        float re = 0.0f, im = 0.0f;
        int idx = 0;
        for (int j = 0; j < n; ++j) {
            fi_cmac<true>(re, im, spec[j * FI_XB + xl], tw[idx]);
            idx += k;
            if (idx >= n) idx -= n;
        }
        if (x0 + xl < inner) g[(int64_t)k * inner + xl] = f32x2{re, im};
    }
}

// 5. grid: fi_row_groups.  out = z + Re(inverse DFT along w); the imaginary part is rounding noise of a real operator and never formed.
template <int UNIT = 0>          // (a template only so that the header may be included by several translation units)
__global__ void __launch_bounds__(FI_THREADS) freeinit_rows_inv_kernel(const AaFreeInit p, const f32x2* ws) {
    const int w = p.w, R = fi_rows_per_group(w);
    const int64_t rows = (int64_t)p.volumes * p.frames * p.h;
    const int64_t row0 = (int64_t)blockIdx.x * R;
    const int count = (int)(rows - row0 < R ? rows - row0 : R) * w;
    const int64_t base = row0 * w;
    const f32x2* tw = fi_stage_table(reinterpret_cast<const f32x2*>(p.twiddle) + fi_tw_w(p), w);
    f32x2* tile = reinterpret_cast<f32x2*>(dyn_smem() + FI_TW_BYTES);
    for (int i = (int)threadIdx.x; i < count; i += FI_THREADS) tile[i] = ws[base + i];
    __syncthreads();
    for (int o = (int)threadIdx.x; o < count; o += FI_THREADS) {
        const int r = o / w, x = o - r * w;
        const f32x2* line = tile + r * w;
        float re = 0.0f;
        int idx = 0;
        for (int k = 0; k < w; ++k) {
            const f32x2 v = line[k], t = tw[idx];
            re += v[0] * t[0];
            re -= v[1] * t[1];
            idx += x;
            if (idx >= w) idx -= w;
        }
        p.out[base + o] = p.z[base + o] + re;
    }
}

}  // namespace aa
