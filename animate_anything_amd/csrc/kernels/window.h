// Context windows (MultiDiffusion over time): per step the UNet runs on overlapping windows of the clip's frames and one solver update
// is applied to the blend of their predictions (aa_mi355.h AaWindow).  Two kernels around the UNet run of one window:
//  * window_gather_kernel  dst[b, c, j, p] = src[b, c, frame[j], p] on the fp32 latents: the window's frames into the session's `sample`
//  * window_merge_kernel   the window's guided prediction - read from the UNet's token matrix exactly as guided_token() (glue.h) reads
//                          it - blended into the clip's merged token matrix through an fp32 accumulator:
//                              first && last    merged = the window's tokens    first && !last   acc = w * guided
//                              !first && !last  acc += w * guided               !first && last   merged = (T)(acc + w * guided)
//                          A frame's first window WRITES the accumulator, so nothing is ever zeroed; its last window rounds once.
//                          Under guidance the merged matrix keeps BOTH halves, [uncond clips | text clips] like a UNet output, and the
//                          step kernel reads it with the same guidance: a frame held by one window hands u and t through bit for bit
//                          (the step then forms u + g (t - u) in fp32 from the bits the unwindowed step would read); a blended frame
//                          stores its value c in both halves, and c + g (c - c) is c exactly.  Guidance off: one half.
// The slot j of a workgroup is blockIdx.y: frame, weight and the two flags are wave-uniform (scalar loads from the descriptor, uniform
// branches).  A thread owns one token: at 4 channels one 8-byte load and one 8-byte store per guidance half, one 16-byte accumulator
// access (VEC); any channel count 1..8 and any pitch / alignment element by element.  A launch touches each (clip, frame, pixel) once
// and launches are ordered by the stream: no atomics, and a replay repeats the bits.
#pragma once
#include "dev.h"
#include "aa_mi355.h"

namespace aa {

constexpr int WIN_THREADS = 256;
constexpr int WIN_MAX_CHANNELS = 8;

// grid (ceil(hw / (VEC ? 4 : 1) / 256), window_frames, clips * channels); VEC: hw % 4 == 0 and 16-byte aligned pointers
template <bool VEC>
__global__ void __launch_bounds__(WIN_THREADS) window_gather_kernel(const AaWindowGather p) {
    const int j = (int)blockIdx.y;
    const int64_t plane = (int64_t)blockIdx.z;                                           // clip * channels + channel
    const float* src = p.src + (plane * p.total_frames + p.window.frame[j]) * p.hw;
    float* dst = p.dst + (plane * p.window.window_frames + j) * p.hw;
    const int i = (int)blockIdx.x * WIN_THREADS + (int)threadIdx.x;
    if constexpr (VEC) {
        if (i < (p.hw >> 2)) reinterpret_cast<f32x4*>(dst)[i] = reinterpret_cast<const f32x4*>(src)[i];
    } else {
        if (i < p.hw) dst[i] = src[i];
    }
}

// grid (ceil(hw / 256), window_frames, clips)
template <typename T, bool VEC>
__global__ void __launch_bounds__(WIN_THREADS) window_merge_kernel(const AaWindowMerge p) {
    const int pix = (int)blockIdx.x * WIN_THREADS + (int)threadIdx.x;
    if (pix >= p.hw) return;
    const int j = (int)blockIdx.y, b = (int)blockIdx.z;
    const int W1 = p.window.window_frames + 1, T1 = p.total_frames + 1;
    const int f = p.window.frame[j];
    const float w = p.window.weight[j];
    const bool first = p.window.first[j] != 0, last = p.window.last[j] != 0;
    const bool guided = p.guidance_on != 0;
    const T* tok = reinterpret_cast<const T*>(p.tokens);
    const T* pu = tok + (((int64_t)b * W1 + j + 1) * p.hw + pix) * p.ld;                  // frame 0 of the UNet output is dropped
    const T* pt = tok + (((int64_t)(p.clips + b) * W1 + j + 1) * p.hw + pix) * p.ld;      // [uncond clips | text clips]
    float* acc = p.acc + (((int64_t)b * p.total_frames + f) * p.hw + pix) * p.channels;
    T* ou = reinterpret_cast<T*>(p.merged) + (((int64_t)b * T1 + f + 1) * p.hw + pix) * p.out_ld;
    T* ot = reinterpret_cast<T*>(p.merged) + (((int64_t)(p.clips + b) * T1 + f + 1) * p.hw + pix) * p.out_ld;   // written under guidance only
    if constexpr (VEC) {                                                                 // channels == 4
        union Pack4 { u32x2 raw; T e[4]; };
        Pack4 u, t, o;
        u.raw = *reinterpret_cast<const u32x2*>(pu);
        if (guided) t.raw = *reinterpret_cast<const u32x2*>(pt);
        if (first && last) {                                                             // the window's bits, both halves
            *reinterpret_cast<u32x2*>(ou) = u.raw;
            if (guided) *reinterpret_cast<u32x2*>(ot) = t.raw;
            return;
        }
        float g[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float uc = (float)u.e[c];
            g[c] = guided ? uc + p.guidance * ((float)t.e[c] - uc) : uc;
        }
        if (first) {
            *reinterpret_cast<f32x4*>(acc) = f32x4{w * g[0], w * g[1], w * g[2], w * g[3]};
            return;
        }
        const f32x4 a = *reinterpret_cast<const f32x4*>(acc);
        const f32x4 s = {a[0] + w * g[0], a[1] + w * g[1], a[2] + w * g[2], a[3] + w * g[3]};
        if (last) {
#pragma unroll
            for (int c = 0; c < 4; ++c) o.e[c] = (T)s[c];
            *reinterpret_cast<u32x2*>(ou) = o.raw;
            if (guided) *reinterpret_cast<u32x2*>(ot) = o.raw;
        } else {
            *reinterpret_cast<f32x4*>(acc) = s;
        }
    } else {
        for (int c = 0; c < p.channels; ++c) {
            const T ub = pu[c];
            const float uc = (float)ub;
            if (first && last) {
                ou[c] = ub;
                if (guided) ot[c] = pt[c];
                continue;
            }
            const float g = guided ? uc + p.guidance * ((float)pt[c] - uc) : uc;
            if (first) acc[c] = w * g;
            else if (last) {
                const T v = (T)(acc[c] + w * g);
                ou[c] = v;
                if (guided) ot[c] = v;
            } else acc[c] += w * g;
        }
    }
}

}  // namespace aa
