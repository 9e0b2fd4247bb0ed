// The transformer device code that the frozen encoders share: transformer.hip (SBERT_ENCODER's RoBERTa forward) and clip.hip (the two CLIP
// towers) include this file, launch these kernels from their own entry points and instantiate only what they launch.
//
//   ln_row_store       LayerNorm of a row held by one wave: f32 two-pass statistics, an f32 store and an optional 16-bit copy
//   attention_kernel   softmax(Q K^T / sqrt(64) + mask) V per (sample, head) for T <= 64; the mask is the key padding of `lens`, or causal
//   bias_act_kernel    x + bias through erf-GELU or QuickGELU, streaming in 8-element units
//
// Forward only, no atomics: every output element has one writer and a fixed summation order.
#pragma once
#include "common.h"

namespace {

constexpr int LN_MAXU = 4;          // 16-byte units per lane: rows of up to 64 * 4 * 4 = 1024 floats
constexpr int AT_D = 64;            // head dimension
constexpr int AT_T = 64;            // longest sequence of the attention kernel
constexpr int ACT_GELU = 0;         // exact (erf) GELU
constexpr int ACT_QUICK_GELU = 1;   // v * sigmoid(1.702 v)

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
inline unsigned row_grid(int64_t rows) { return (unsigned)((rows + 3) / 4 < 8192 ? (rows + 3) / 4 : 8192); }
inline bool ln_width(int H) { return H >= 64 && H % 64 == 0 && H <= 256 * LN_MAXU; }

// LayerNorm of the row a wave holds as v[k] = unit (lane + 64 k); writes f32 and, if asked, the 16-bit copy
__device__ __forceinline__ void ln_row_store(f32x4 (&v)[LN_MAXU], int lane, int H4, int H, const f32x4* __restrict__ gamma,
                                             const f32x4* __restrict__ beta, float eps, f32x4* __restrict__ out,
                                             bf16x4* __restrict__ out16) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < LN_MAXU; ++k)
        if (lane + 64 * k < H4) s += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);
    const float mean = wave_sum(s) / (float)H;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < LN_MAXU; ++k)
        if (lane + 64 * k < H4) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[k][i] -= mean;
                q += v[k][i] * v[k][i];
            }
        }
    const float rstd = 1.f / sqrtf(wave_sum(q) / (float)H + eps);
#pragma unroll
    for (int k = 0; k < LN_MAXU; ++k) {
        const int u = lane + 64 * k;
        if (u < H4) {
            const f32x4 g = gamma[u], b = beta[u];
            f32x4 y;
            bf16x4 yh;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                y[i] = v[k][i] * rstd * g[i] + b[i];
                yh[i] = (xmc_h16)y[i];
            }
            out[u] = y;
            if (out16) out16[u] = yh;
        }
    }
}

// one workgroup = one (sample, head); qkv rows are [Q (H) | K (H) | V (H)], head h in columns [64 h, 64 h + 64) of each.
// CAUSAL: query r sees keys 0 .. r of a full-length sample (`lens` is not read); else the first lens[b] keys, and padded queries give zeros
template <int ODT, bool CAUSAL>
__global__ __launch_bounds__(256) void attention_kernel(const float* __restrict__ qkv, const int32_t* __restrict__ lens,
                                                        void* __restrict__ out, int T, int H) {
    // LDS sized by T, not by the longest sequence the kernel takes: at T = 20 a workgroup holds 15 KiB and eight of them share a CU
    extern __shared__ __attribute__((aligned(16))) float at_smem[];
    float (*q_s)[AT_D] = reinterpret_cast<float (*)[AT_D]>(at_smem);                          // [T][64]
    float (*v_s)[AT_D] = reinterpret_cast<float (*)[AT_D]>(at_smem + (size_t)T * AT_D);       // [T][64]
    float (*k_s)[AT_D + 1] = reinterpret_cast<float (*)[AT_D + 1]>(at_smem + (size_t)2 * T * AT_D);   // [T][65]: read with the key on the lane,
                                                                                              // odd row stride, no bank conflict
    const int b = blockIdx.x, head = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int len = CAUSAL ? T : min(max(lens[b], 0), T);
    const float* base = qkv + (size_t)b * T * 3 * H + head * AT_D;
    for (int i = tid; i < len * (AT_D / 4); i += 256) {
        const int t = i / (AT_D / 4), c = (i % (AT_D / 4)) * 4;
        const float* r = base + (size_t)t * 3 * H + c;
        const f32x4 q = *reinterpret_cast<const f32x4*>(r), k = *reinterpret_cast<const f32x4*>(r + H),
                    v = *reinterpret_cast<const f32x4*>(r + 2 * H);
        *reinterpret_cast<f32x4*>(&q_s[t][c]) = q;
        *reinterpret_cast<f32x4*>(&v_s[t][c]) = v;
        k_s[t][c] = k[0], k_s[t][c + 1] = k[1], k_s[t][c + 2] = k[2], k_s[t][c + 3] = k[3];
    }
    __syncthreads();
    for (int r = wave; r < T; r += 4) {                       // (wave-uniform trip count and branches)
        float o = 0.f;
        if (CAUSAL || r < len) {
            const int keys = CAUSAL ? r + 1 : len;            // causal: key 0 is always there, so the row is finite
            // scores: lane j holds key j
            float s = 0.f;
            if (lane < keys) {
#pragma unroll
                for (int d = 0; d < AT_D; d += 4) {
                    const f32x4 q = *reinterpret_cast<const f32x4*>(&q_s[r][d]);
                    s += q[0] * k_s[lane][d] + q[1] * k_s[lane][d + 1] + q[2] * k_s[lane][d + 2] + q[3] * k_s[lane][d + 3];
                }
                s *= 0.125f;                                  // 1 / sqrt(64)
            }
            const float m = wave_max(lane < keys ? s : -INFINITY);
            const float p = lane < keys ? expf(s - m) : 0.f;  // keys out of sight: excluded
            const float l = wave_sum(p);
            // context: lane d holds channel d; p of key j comes out of lane j's register (j is wave-uniform)
            for (int j = 0; j < keys; ++j)
                o += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, p), j)) * v_s[j][lane];
            o /= l;
        }
        // rows of padded queries: zero (they are dropped by the pooling tail)
        const size_t idx = ((size_t)b * T + r) * H + head * AT_D + lane;
        if (ODT == XMC_F32) reinterpret_cast<float*>(out)[idx] = o;
        else reinterpret_cast<xmc_h16*>(out)[idx] = (xmc_h16)o;
    }
}

template <int ODT, int ACT>
__global__ __launch_bounds__(256) void bias_act_kernel(const float* __restrict__ x, const float* __restrict__ bias,
                                                       void* __restrict__ out, int64_t n8, int F8) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
        float v[8], bv[8];
        Vec8<XMC_F32>::load(x, (size_t)i, v);
        Vec8<XMC_F32>::load(bias, (size_t)(i % F8), bv);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float a = v[k] + bv[k];
            if (ACT == ACT_GELU) v[k] = 0.5f * a * (1.f + erff(a * 0.70710678118654752f));
            else v[k] = a / (1.f + expf(-1.702f * a));        // a -> -inf: exp overflows to +inf and the quotient is -0, never a NaN
        }
        Vec8<ODT>::store(out, (size_t)i, v);
    }
}

}  // namespace
