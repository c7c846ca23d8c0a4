// W8A8 linear layers in OCP e4m3 (see include/aa_mi355.h: aa_quant_rows_fp8, aa_linear_fp8): the FeedForward pair of the 640- / 1280-channel
// transformers (diffusers GEGLU.proj: C -> 8C and FeedForward.net[2]: 4C -> C; reference models/unet_3d_blocks.py via diffusers) as an opt-in
// path below 16 bits.
//  * quant_rows_fp8_kernel: one wave per token row; the row sits in registers (16 elements per lane and piece: 2 x 16-byte loads, one 16-byte
//    store), optionally LayerNorm'ed there (fp32 statistics, two passes over the registers), then
//        s = max(absmax(row), AA_FP8_TINY) / 448,   q = e4m3(clamp(x * (448 / max(absmax, tiny)), -448, 448))  (round to nearest even)
//    - the clamp keeps the conversion away from the NaN encodings 0x7F / 0xFF whatever the product's last bit does;
//  * linear_fp8_kernel: Y = (Aq Wq^T) sa[m] sw[n] + bias over 128 x 128 tiles, four waves as 2 x 2, every wave 2 x 2 blocks of the block-scaled
//    v_mfma_scale_f32_32x32x64_f8f6f4 with both block scales 1.0 (E8M0 127): the real scales are per ROW / per CHANNEL, not per 32 k, and are
//    applied in the fp32 epilogue.  The weights are the MFMA "A" operand (rows -> accumulator registers), the tokens the "B" operand (columns ->
//    lanes); ops.pack_weight_fp8 orders the 32 weight rows of a block so that a lane's 16 registers are 16 CONSECUTIVE output channels (two
//    16-byte stores).  K runs in stages of 128 bytes per row: both operand tiles (16 KB each) arrive by LDS-DMA as 8-row x 128-byte pieces (whole
//    cache lines), 16-byte slots XOR-swizzled with (row & 7) on the SOURCE side; two LDS buffers, one barrier per stage, stage t + 1 in flight
//    under the MFMAs of stage t.  Rows behind M and weight rows behind N are fetched as zeros by the buffer range check (offset bit 31) and never
//    stored; a lane behind the last row reads no scale and no residual.
//    The two 32-byte halves of a lane's fragment are k = 32 h .. 32 h + 31 of the 64-deep step for BOTH operands (the layout the emulator
//    stand-in below restates); a product only needs the two operands to agree on it.
//  * geglu: ops.pack_weight_fp8(geglu=True) alternates blocks of 32 value rows / 32 gate rows, a wave's two column blocks are value and gate of
//    the same 32 channels: out[M, N / 2] = value * gelu_erf(gate) in registers (conv_gemm.h gelu_erf_f, the library's fast-math form).
#pragma once
#include "dev.h"
#include "aa_mi355.h"
#include "conv_gemm.h"      // gelu_erf_f
#include "norm.h"           // wave_sum, wave_max

#if !defined(__HIPCC__)
// ---- host stand-ins (emulator build) of the two device primitives this file adds to device/dev.h --------------------------------------------
inline float emu_e4m3_to_f32(unsigned b) {
    const int e = (b >> 3) & 15, m = b & 7;
    const float v = e == 0 ? std::ldexp((float)m, -9) : std::ldexp(1.0f + (float)m / 8.0f, e - 7);
    return (b & 0x80u) ? -v : v;
}
// |v| <= 448, round to nearest even; below 2^-6 the grid is 2^-9 (byte = multiples of it; 8 of them are the smallest normal number, byte 0x08)
inline unsigned emu_f32_to_e4m3(float v) {
    const unsigned sign = std::signbit(v) ? 0x80u : 0u;
    const float a = std::fabs(v);
    if (a < 0.015625f) return sign | (unsigned)std::nearbyint(std::ldexp(a, 9));
    int e;
    const float f = std::frexp(a, &e);                      // a = f 2^e, f in [0.5, 1)
    e -= 1;
    int m = (int)std::nearbyint((2.0f * f - 1.0f) * 8.0f);
    if (m == 8) { m = 0; ++e; }
    return sign | (unsigned)((e + 7) << 3) | (unsigned)m;
}
inline unsigned cvt4_e4m3(float a, float b, float c, float d) {
    return emu_f32_to_e4m3(a) | (emu_f32_to_e4m3(b) << 8) | (emu_f32_to_e4m3(c) << 16) | (emu_f32_to_e4m3(d) << 24);
}
// D = A(32 x 64) B(64 x 32) + C, e4m3 operands, block scales 1: lane l supplies row (l & 31) of A and column (l & 31) of B, bytes
// k = 32 (l >> 5) .. + 31 (lo = the first 16); D as every 32 x 32 form: col = l & 31, row = (r & 3) + 8 (r >> 2) + 4 (l >> 5)
inline f32x16 mfma_scale_32x32x64_e4m3(u32x4 a_lo, u32x4 a_hi, u32x4 b_lo, u32x4 b_hi, f32x16 c) {
    struct Ops { unsigned char a[32], b[32]; } mine;
    std::memcpy(mine.a, &a_lo, 16); std::memcpy(mine.a + 16, &a_hi, 16);
    std::memcpy(mine.b, &b_lo, 16); std::memcpy(mine.b + 16, &b_hi, 16);
    f32x16 d = c;
    emu::wave_collective(&mine, [&](const std::vector<const void*>& s) {
        const int lane = emu::linear_tid() & 63, j = lane & 31;
        for (int r = 0; r < 16; ++r) {
            const int i = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            float acc = c[r];
            for (int half = 0; half < 2; ++half) {
                const Ops* pa = static_cast<const Ops*>(s[i + 32 * half]);
                const Ops* pb = static_cast<const Ops*>(s[j + 32 * half]);
                for (int e = 0; e < 32; ++e) acc += emu_e4m3_to_f32(pa->a[e]) * emu_e4m3_to_f32(pb->b[e]);
            }
            d[r] = acc;
        }
    });
    return d;
}
#endif

namespace aa {

constexpr float FP8_MAX = 448.0f;                 // largest finite e4m3fn value (byte 0x7E)
constexpr float FP8_TINY = 1e-12f;                // include/aa_mi355.h: AA_FP8_TINY (an all-zero row: zeros and the scale tiny / 448)

// J = 16-element pieces per lane: K <= 1024 J
template <typename T, int J>
__global__ void __launch_bounds__(256) quant_rows_fp8_kernel(const AaQuantRowsFp8 p) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.rows) return;                    // (whole waves: the collectives below never wait for a missing lane)
    const int K = p.channels;
    const T* x = static_cast<const T*>(p.x) + row * p.ldx;
    float v[J][16];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int k0 = (lane + 64 * j) * 16;
        Pack8<T> a, b;
        a.raw = u32x4{0u, 0u, 0u, 0u}; b.raw = u32x4{0u, 0u, 0u, 0u};
        if (k0 < K) {
            a.raw = *reinterpret_cast<const u32x4*>(x + k0);
            b.raw = *reinterpret_cast<const u32x4*>(x + k0 + 8);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) { v[j][e] = (float)a.e[e]; v[j][8 + e] = (float)b.e[e]; }
    }
    if (p.gamma) {
        float sum = 0.0f;
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) sum += v[j][e];                          // (pieces past the row hold zeros)
        const float mean = wave_sum(sum) / (float)K;
        float sq = 0.0f;
#pragma unroll
        for (int j = 0; j < J; ++j)
            if ((lane + 64 * j) * 16 < K) {
#pragma unroll
                for (int e = 0; e < 16; ++e) { const float d = v[j][e] - mean; sq += d * d; }
            }
        const float rstd = rsqrtf(wave_sum(sq) / (float)K + p.ln_eps);
        const T* gamma = static_cast<const T*>(p.gamma);
        const T* beta = static_cast<const T*>(p.beta);
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int k0 = (lane + 64 * j) * 16;
            if (k0 < K) {
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    Pack8<T> g, b;
                    g.raw = *reinterpret_cast<const u32x4*>(gamma + k0 + 8 * hh);
                    b.raw = u32x4{0u, 0u, 0u, 0u};
                    if (beta) b.raw = *reinterpret_cast<const u32x4*>(beta + k0 + 8 * hh);
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[j][8 * hh + e] = (v[j][8 * hh + e] - mean) * rstd * (float)g.e[e] + (float)b.e[e];
                }
            }
        }
    }
    float amax = 0.0f;
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) amax = fmaxf(amax, fabsf(v[j][e]));
    amax = fmaxf(wave_max(amax), FP8_TINY);
    const float inv = FP8_MAX / amax;
    if (lane == 0) p.scale[row] = amax / FP8_MAX;
    unsigned char* q = static_cast<unsigned char*>(p.q) + row * p.ldq;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int k0 = (lane + 64 * j) * 16;
        if (k0 < K) {
            u32x4 o;
#pragma unroll
            for (int w = 0; w < 4; ++w)
                o[w] = cvt4_e4m3(clamp_f(v[j][4 * w] * inv, -FP8_MAX, FP8_MAX), clamp_f(v[j][4 * w + 1] * inv, -FP8_MAX, FP8_MAX),
                                 clamp_f(v[j][4 * w + 2] * inv, -FP8_MAX, FP8_MAX), clamp_f(v[j][4 * w + 3] * inv, -FP8_MAX, FP8_MAX));
            *reinterpret_cast<u32x4*>(q + k0) = o;
        }
    }
}

constexpr int L8_BM = 128, L8_BN = 128, L8_BK = 128;          // tile rows (tokens), columns (output channels), bytes of K per stage
constexpr int L8_TILE_BYTES = 128 * L8_BK;                    // one operand tile of a stage: [128 rows][128 bytes]
constexpr int L8_LDS_BYTES = 4 * L8_TILE_BYTES;               // (tokens, weights) x two buffers
constexpr int L8_GROUP_M = 8;                                 // tile order: 8 row tiles x all column tiles, row tiles fastest

template <typename T, bool GEGLU>
__global__ void __launch_bounds__(256, 2) linear_fp8_kernel(const AaLinearFp8 p, const int tiles_m, const int tiles_n) {
    constexpr unsigned OOB = 0x80000000u;
    char* lds = dyn_smem();
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = wave_id();
    const int wm = wave >> 1, wn = wave & 1;                  // the wave's 64 tokens x 64 channels of the tile
    const int c = lane & 31, h = lane >> 5;

    // XCD-aware tile order (conv_gemm.h): consecutive workgroup ids go round the 8 XCDs, so every XCD gets a contiguous run of logical tiles;
    // inside a run, L8_GROUP_M row tiles share a weight panel before the next panel starts (the panel and the 8 token tiles stay in that L2)
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int xq = nwg >> 3, xr = nwg & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    const int logical = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + idx;
    const int group = logical / (L8_GROUP_M * tiles_n);
    const int first_m = group * L8_GROUP_M;
    const int gsz = tiles_m - first_m < L8_GROUP_M ? tiles_m - first_m : L8_GROUP_M;
    const int rem = logical - group * L8_GROUP_M * tiles_n;
    const int tile_m = first_m + rem % gsz, tile_n = rem / gsz;
    const int64_t m0 = (int64_t)tile_m * L8_BM;
    const int n0 = tile_n * L8_BN;

    const int K = p.k;
    const int nk = K / L8_BK;
    const BufRsrc r_a = make_rsrc(p.a, (unsigned)(p.rows * K));
    const BufRsrc r_w = make_rsrc(p.w, (unsigned)((int64_t)p.n * K));

    // ---- staging: piece pi = wave + 4 j (j < 4) of an operand tile = its rows 8 pi .. 8 pi + 7; lane = (row l >> 3, 16-byte slot l & 7) fetches
    // source slot (l & 7) ^ (row & 7): LDS slot s of row r holds source slot s ^ (r & 7)
    unsigned off_a[4], off_w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = 8 * (wave + 4 * j) + (lane >> 3);
        const unsigned slot = (unsigned)(((lane & 7) ^ (r & 7)) << 4);
        const int64_t ra = m0 + r;
        const int rw = n0 + r;
        off_a[j] = ra < p.rows ? (unsigned)(ra * K) + slot : OOB;
        off_w[j] = rw < p.n ? (unsigned)((int64_t)rw * K) + slot : OOB;
    }
    auto stage = [&](int t) __attribute__((always_inline)) {
        char* buf = lds + (t & 1) * 2 * L8_TILE_BYTES;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            async_copy16_buf_s(r_a, off_a[j], (unsigned)(t * L8_BK), buf + (wave + 4 * j) * 1024);
            async_copy16_buf_s(r_w, off_w[j], (unsigned)(t * L8_BK), buf + L8_TILE_BYTES + (wave + 4 * j) * 1024);
        }
    };
    // ---- fragments: block row c of a 32-row block, k-step ks (64 bytes), half h: source slots 4 ks + 2 h, + 1
    unsigned fa[2][2];                                        // [k-step][lo / hi]: byte offset inside a 32-row block of a tile
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < 2; ++i) fa[ks][i] = (unsigned)(c * L8_BK + (((4 * ks + 2 * h + i) ^ (c & 7)) << 4));

    f32x16 acc[2][2];                                         // [token block][channel block]
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mb][nb][e] = 0.0f;

    stage(0);
    for (int t = 0; t < nk; ++t) {
        dma_wait<0>();                                        // this wave's pieces of stage t have landed ...
        block_barrier();                                      // ... everyone's have, and everyone is done reading the other buffer (stage t - 1)
        if (t + 1 < nk) stage(t + 1);
        const char* ta = lds + (t & 1) * 2 * L8_TILE_BYTES + (64 * wm) * L8_BK;
        const char* tw = lds + (t & 1) * 2 * L8_TILE_BYTES + L8_TILE_BYTES + (64 * wn) * L8_BK;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            u32x4 xa[2][2], xw[2][2];                         // [block][lo / hi]
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    lds_read16_async(xa[b][i], ta + b * 32 * L8_BK + fa[ks][i]);
                    lds_read16_async(xw[b][i], tw + b * 32 * L8_BK + fa[ks][i]);
                }
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int i = 0; i < 2; ++i) { lds_wait<0>(xa[b][i]); lds_wait<0>(xw[b][i]); }
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb)
                    acc[mb][nb] = mfma_scale_32x32x64_e4m3(xw[nb][0], xw[nb][1], xa[mb][0], xa[mb][1], acc[mb][nb]);
        }
    }

    // ---- epilogue in registers: lane = token c of a block, registers = channels 16 h .. 16 h + 15 of a 32-channel block (pack_weight_fp8's row order)
    const int nw0 = n0 + 64 * wn;                             // the wave's first (packed) channel
    if (nw0 >= p.n) return;                                   // (N is a multiple of 64: a wave's columns are all real or all padding)
    const BufRsrc r_o = make_rsrc(p.out, (unsigned)(p.rows * p.ldo * 2));
    const BufRsrc r_res = make_rsrc(p.residual, p.residual ? (unsigned)(p.rows * p.ld_res * 2) : 0u);
    float sw[2][16], bs[2][16];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int e4 = 0; e4 < 4; ++e4) {
            const int n = nw0 + 32 * nb + 16 * h + 4 * e4;
            const f32x4 s4 = *reinterpret_cast<const f32x4*>(p.w_scale + n);
            const f32x4 b4 = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + n) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int e = 0; e < 4; ++e) { sw[nb][4 * e4 + e] = s4[e]; bs[nb][4 * e4 + e] = b4[e]; }
        }
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
        const int64_t m = m0 + 64 * wm + 32 * mb + c;
        const bool row_ok = m < p.rows;
        const float sa = row_ok ? p.a_scale[m] : 0.0f;
        if constexpr (GEGLU) {
            // block 0 = value, block 1 = gate of output channels nw0 / 2 + 16 h ..
            const unsigned ob = row_ok ? (unsigned)((m * p.ldo + (nw0 >> 1) + 16 * h) * 2) : OOB;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                Pack8<T> o;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int r = 8 * half + e;
                    const float val = acc[mb][0][r] * (sa * sw[0][r]) + bs[0][r];
                    const float gate = acc[mb][1][r] * (sa * sw[1][r]) + bs[1][r];
                    o.e[e] = (T)(val * gelu_erf_f(gate));
                }
                buf_store16(r_o, ob + 16 * half, o.raw);
            }
        } else {
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                const int n = nw0 + 32 * nb + 16 * h;
                const unsigned ob = row_ok ? (unsigned)((m * p.ldo + n) * 2) : OOB;
                const unsigned rb = row_ok && p.residual ? (unsigned)((m * p.ld_res + n) * 2) : OOB;
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    Pack8<T> o, res;
                    res.raw = buf_load16(r_res, rb + 16 * half);              // (no residual: a zero-length descriptor, zeros)
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int r = 8 * half + e;
                        o.e[e] = (T)(acc[mb][nb][r] * (sa * sw[nb][r]) + bs[nb][r] + (float)res.e[e]);
                    }
                    buf_store16(r_o, ob + 16 * half, o.raw);
                }
            }
        }
    }
}

}  // namespace aa
