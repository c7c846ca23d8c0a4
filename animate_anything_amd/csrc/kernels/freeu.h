// FreeU (Si et al., "FreeU: Free Lunch in Diffusion U-Net"; diffusers 0.24 `apply_freeu` + `fourier_filter(threshold=1)`) on the two
// operands of an up-block resnet, in the UNet's channels-last token layout, as ONE launch:
//  * hidden [images*h*w, c_hidden]: columns [0, c_hidden/2) times b
//  * skip   [images*h*w, c_skip]:   per (image, channel) plane  y = x + (s - 1) * Re(P x), P the projector on the Fourier modes
//                                   {0, h-1} x {0, w-1} (the 2x2 centre of the shifted spectrum).  With ty = 2 pi row / h, tx = 2 pi col / w
//                                   Re(P x) = (1 / hw) * sum_k (sum_pixels x * phi_k) * phi_k  over the seven real functions
//                                   1, cos ty, sin ty, cos tx, sin tx, cos(ty + tx), sin(ty + tx)  (DESIGN.md section 10): no FFT.
// cos / sin come from a host-built fp32 table [hw][4] = (cos ty, sin ty, cos tx, sin tx), zero along a 1-pixel axis (the modes of that axis
// coincide; the zeros take the duplicates out of the sum).
#pragma once
#include "dev.h"
#include "aa_mi355.h"

namespace aa {

constexpr int FU_CG = 8;                       // 16-byte channel chunks per workgroup (64 channels = one 128-byte line per pixel)
constexpr int FU_PL = 256 / FU_CG;             // pixel lanes: thread t owns chunk t & 7 and the pixels (t >> 3) + 32 i
constexpr int FU_KEEP = 8;                     // pixels per thread kept in registers between the sums and the apply (planes up to 256 pixels
                                               // are read once; a longer plane re-reads the rest - a loop, at most twice per element)
constexpr int FU_LDS_BYTES = 5 * FU_CG * 56 * 4;      // four waves' partial sums + the totals

AA_HD inline int fu_skip_blocks(const AaFreeU& p) {
    return (p.s == 1.0f && p.skip == p.skip_out) ? 0 : p.images * ((p.c_skip / 8 + FU_CG - 1) / FU_CG);
}

// the seven sums of one pixel's 8 channels, k-major, always in this order
template <typename T>
__device__ __forceinline__ void fu_accumulate(float (&acc)[7][8], const u32x4& raw, const f32x4& t) {
    Pack8<T> v;
    v.raw = raw;
    const float c5 = t[0] * t[2] - t[1] * t[3], c6 = t[1] * t[2] + t[0] * t[3];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float x = (float)v.e[e];
        acc[0][e] += x;
        acc[1][e] += x * t[0];
        acc[2][e] += x * t[1];
        acc[3][e] += x * t[2];
        acc[4][e] += x * t[3];
        acc[5][e] += x * c5;
        acc[6][e] += x * c6;
    }
}

template <typename T>
__device__ __forceinline__ u32x4 fu_apply(const float (&a)[7][8], const u32x4& raw, const f32x4& t) {
    Pack8<T> v, o;
    v.raw = raw;
    const float c5 = t[0] * t[2] - t[1] * t[3], c6 = t[1] * t[2] + t[0] * t[3];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float y = (float)v.e[e] + a[0][e];
        y += a[1][e] * t[0];
        y += a[2][e] * t[1];
        y += a[3][e] * t[2];
        y += a[4][e] * t[3];
        y += a[5][e] * c5;
        y += a[6][e] * c6;
        o.e[e] = (T)y;                         // the one rounding to the storage type
    }
    return o.raw;
}

// Workgroups [0, fu_skip_blocks) filter the skip tensor, one (image, 64-channel group) each; the rest scale the hidden tensor
// (grid-stride over 16-byte chunks).  No atomics, every sum in a fixed order: a replay reproduces an eager run bit for bit.
// In place (out == in, same pitch) is safe: a thread writes only elements it has read itself, behind the workgroup's barrier.
// (launch bounds: four waves per SIMD = 128 registers; hipcc takes 126 without scratch.  Left to itself it hoists every load of the unrolled
// part and takes 272, one wave per SIMD.)
template <typename T>
__global__ void __launch_bounds__(256, 4) freeu_tok_kernel(const AaFreeU p) {
    const int tid = (int)threadIdx.x;
    const int skip_blocks = fu_skip_blocks(p);
    if ((int)blockIdx.x >= skip_blocks) {
        // ---- hidden: columns [0, c_hidden / 2) * b; in place only the chunks that hold such a column are touched
        const T* in = reinterpret_cast<const T*>(p.hidden);
        T* out = reinterpret_cast<T*>(p.hidden_out);
        const int half = p.c_hidden >> 1;
        const int cpr = (p.hidden == p.hidden_out) ? (half + 7) >> 3 : p.c_hidden >> 3;
        const int64_t total = (int64_t)p.images * p.h * p.w * cpr;
        const int64_t stride = (int64_t)((int)gridDim.x - skip_blocks) * 256;
        for (int64_t c = (int64_t)((int)blockIdx.x - skip_blocks) * 256 + tid; c < total; c += stride) {
            const int64_t r = c / cpr;
            const int n = (int)(c - r * cpr) * 8;
            Pack8<T> v;
            v.raw = *reinterpret_cast<const u32x4*>(in + r * p.hidden_ld + n);
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (n + e < half) v.e[e] = (T)((float)v.e[e] * p.b);
            *reinterpret_cast<u32x4*>(out + r * p.hidden_out_ld + n) = v.raw;
        }
        return;
    }
    // ---- skip
    const int hw = p.h * p.w;
    const int chunks = p.c_skip >> 3;
    const int groups = (chunks + FU_CG - 1) / FU_CG;
    const int img = (int)blockIdx.x / groups;
    const int cl = tid & (FU_CG - 1), pl = tid >> 3;
    const int chunk = ((int)blockIdx.x - img * groups) * FU_CG + cl;
    const bool live = chunk < chunks;                             // (a thread behind the last chunk reads and writes nothing)
    const T* in = reinterpret_cast<const T*>(p.skip) + (int64_t)img * hw * p.skip_ld + chunk * 8;
    T* out = reinterpret_cast<T*>(p.skip_out) + (int64_t)img * hw * p.skip_out_ld + chunk * 8;
    const f32x4* trig = reinterpret_cast<const f32x4*>(p.trig);

    if (p.s == 1.0f) {                                            // the identity filter (out of place): a copy, signed zeros included
        if (live)
            for (int px = pl; px < hw; px += FU_PL)
                *reinterpret_cast<u32x4*>(out + (int64_t)px * p.skip_out_ld) = *reinterpret_cast<const u32x4*>(in + (int64_t)px * p.skip_ld);
        return;
    }

    float acc[7][8];
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[k][e] = 0.0f;
    u32x4 keep[FU_KEEP];
#pragma unroll
    for (int i = 0; i < FU_KEEP; ++i) {
        const int px = pl + FU_PL * i;
        keep[i] = u32x4{0u, 0u, 0u, 0u};
        if (live && px < hw) {
            keep[i] = *reinterpret_cast<const u32x4*>(in + (int64_t)px * p.skip_ld);
            fu_accumulate<T>(acc, keep[i], trig[px]);
        }
    }
    if (live)
        for (int px = pl + FU_PL * FU_KEEP; px < hw; px += FU_PL)
            fu_accumulate<T>(acc, *reinterpret_cast<const u32x4*>(in + (int64_t)px * p.skip_ld), trig[px]);

    // the 8 pixel lanes of a wave (lane bits 3..5), then the four waves through LDS in the order 0, 1, 2, 3
    float* red = reinterpret_cast<float*>(dyn_smem());
    const int wv = tid >> 6;
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float v = acc[k][e];
            v += wave_shfl_xor(v, 8);
            v += wave_shfl_xor(v, 16);
            v += wave_shfl_xor(v, 32);
            if ((tid & 63) < FU_CG) red[(wv * FU_CG + cl) * 56 + k * 8 + e] = v;
        }
    __syncthreads();
    // 448 totals of the workgroup (waves 0, 1, 2, 3 in this order) times (s - 1) / hw, through LDS again: summing the four partials in
    // every thread would hold 224 of them in registers at once
    const float coef = (p.s - 1.0f) / (float)hw;
    float* tot = red + 4 * FU_CG * 56;
    for (int o = tid; o < FU_CG * 56; o += 256)
        tot[o] = (((red[o] + red[FU_CG * 56 + o]) + red[2 * FU_CG * 56 + o]) + red[3 * FU_CG * 56 + o]) * coef;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[k][e] = tot[cl * 56 + k * 8 + e];
    if (!live) return;
#pragma unroll
    for (int i = 0; i < FU_KEEP; ++i) {
        const int px = pl + FU_PL * i;
        if (px < hw) *reinterpret_cast<u32x4*>(out + (int64_t)px * p.skip_out_ld) = fu_apply<T>(acc, keep[i], trig[px]);
    }
    for (int px = pl + FU_PL * FU_KEEP; px < hw; px += FU_PL)
        *reinterpret_cast<u32x4*>(out + (int64_t)px * p.skip_out_ld) =
            fu_apply<T>(acc, *reinterpret_cast<const u32x4*>(in + (int64_t)px * p.skip_ld), trig[px]);
}

}  // namespace aa
