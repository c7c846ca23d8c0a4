// Known-region blend (blended latent diffusion; the known-region step of inpainting samplers): behind a solver step the region the
// motion mask holds still is overwritten with the known latents noised to the level the sampler has just reached, and behind the VAE
// the known pixels are pasted back (aa_mi355.h AaKeepBlend).  One streaming kernel for both, on fp32 planes x[clips][C][T][hw]:
//     kn  = a * known + s * noise                        (no noise operand: kn = a * known)
//     out = x where m >= 1,  kn where m <= 0,  m * x + (1 - m) * kn otherwise        (fp32)
// The two endpoints are SELECTED, on the stored bits: the library is built with -ffast-math, which may re-associate the blend and takes
// every float for finite, so a float select could be folded into arithmetic.  m == 1 hands x through bit for bit whatever known and
// noise hold (NaN, Inf), m == 0 yields kn whatever x holds.
// The frame is blockIdx.y and clip * C + channel is blockIdx.z: the broadcast indices of `known` (one clip / one frame: the condition
// image) and of `mask` (no channel axis) are wave-uniform.  A thread owns 4 consecutive pixels: 16-byte accesses on the fp32 operands,
// 8-byte ones on fp16 / bf16 operands (VEC: hw % 4 == 0 and every pointer 16-byte aligned); any hw / alignment element by element.
// Every element is read and written by one thread, so `out` may be x itself.  No LDS, no atomics: a replay repeats the bits.
#pragma once
#include "dev.h"
#include "aa_mi355.h"

namespace aa {

constexpr int KEEP_THREADS = 256;

template <typename T>
__device__ __forceinline__ void keep_load4(const T* p, float (&v)[4]) {
    if constexpr (sizeof(T) == 4) {
        const f32x4 r = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = r[e];
    } else {
        union { u32x2 raw; T e[4]; } r;
        r.raw = *reinterpret_cast<const u32x2*>(p);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (float)r.e[e];
    }
}

__device__ __forceinline__ uint32_t keep_blend1(uint32_t x_bits, float k, float n, float m, float a, float s, bool noisy) {
    const float x = __builtin_bit_cast(float, x_bits);
    const float kn = noisy ? a * k + s * n : a * k;
    const uint32_t kn_bits = __builtin_bit_cast(uint32_t, kn);
    const uint32_t mix_bits = __builtin_bit_cast(uint32_t, m * x + (1.0f - m) * kn);
    return m >= 1.0f ? x_bits : m <= 0.0f ? kn_bits : mix_bits;                          // integer selects: nothing for fast-math to fold
}

// grid (ceil(hw / (VEC ? 4 : 1) / 256), frames, clips * channels)
template <typename K, typename M, bool VEC>
__global__ void __launch_bounds__(KEEP_THREADS) keep_blend_kernel(const AaKeepBlend p) {
    const int t = (int)blockIdx.y;
    const int plane = (int)blockIdx.z;                                                   // clip * channels + channel
    const int clip = plane / p.channels, ch = plane - clip * p.channels;
    const int kc = p.known_clips == 1 ? 0 : clip, kt = p.known_frames == 1 ? 0 : t;
    const int mc = p.mask_clips == 1 ? 0 : clip, mt = p.mask_frames == 1 ? 0 : t;
    const int64_t row = ((int64_t)plane * p.frames + t) * p.hw;
    const float* x = p.x + row;
    float* out = p.out + row;
    const bool noisy = p.noise != nullptr;
    const float* noise = noisy ? p.noise + row : nullptr;
    const K* known = reinterpret_cast<const K*>(p.known) + (((int64_t)kc * p.channels + ch) * p.known_frames + kt) * p.hw;
    const M* mask = reinterpret_cast<const M*>(p.mask) + ((int64_t)mc * p.mask_frames + mt) * p.hw;
    const int i = (int)blockIdx.x * KEEP_THREADS + (int)threadIdx.x;
    if constexpr (VEC) {
        if (i >= (p.hw >> 2)) return;
        const u32x4 xb = reinterpret_cast<const u32x4*>(x)[i];
        float k[4], m[4], n[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        keep_load4(known + 4 * i, k);
        keep_load4(mask + 4 * i, m);
        if (noisy) keep_load4(noise + 4 * i, n);
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = keep_blend1(xb[e], k[e], n[e], m[e], p.a, p.s, noisy);
        reinterpret_cast<u32x4*>(out)[i] = o;
    } else {
        if (i >= p.hw) return;
        const uint32_t xb = reinterpret_cast<const uint32_t*>(x)[i];
        reinterpret_cast<uint32_t*>(out)[i] = keep_blend1(xb, (float)known[i], noisy ? noise[i] : 0.0f, (float)mask[i], p.a, p.s, noisy);
    }
}

}  // namespace aa
