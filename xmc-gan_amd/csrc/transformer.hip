// Frozen sentence encoder of the SBERT presets: the forward of a RoBERTa encoder (post-LayerNorm transformer layers) around the
// MFMA GEMMs of the 1x1 convolution path, and the pooling tail of SBERT_ENCODER.forward (reference model/encoder.py:50-70).
// Forward only, no atomics anywhere: every output element has one writer and a fixed summation order.
//
//   xmc_roberta_embed_ln   word[ids] + position[pos] + token_type[0], LayerNorm; pos = t + 1 + pad for t < len, pad beyond
//                          (cumsum(mask) * mask + padding_idx of a right-padded batch).  One wave per token row.
//   xmc_add_layernorm      LN(x [+ bias] + residual): one wave per row, the row in registers (16-byte units), f32 two-pass statistics
//   xmc_attention_short    softmax(Q K^T / sqrt(64) + key padding mask) V per (sample, head) for T <= 64: Q, K, V of the head in LDS,
//                          one wave per query row, the key on the lane for the scores and the channel on the lane for P V
//                          (P stays in registers: v_readlane of the wave-uniform key index)
//   xmc_bias_gelu          x + bias, exact (erf) GELU, streaming in 8-element units
//   xmc_sbert_pool         mask, transpose to [B, H, L], masked mean, optional L2 normalisation: one workgroup per sample
//
// Every kernel is bandwidth- or latency-bound (the encoder's FLOPs are in its four GEMMs per layer); the residual stream, the
// statistics, the softmax and the pooling are f32 in every precision mode, and the kernels that feed a GEMM can write a second copy
// of their result in the build's 16-bit format so that no cast launch sits between them and the GEMM.
#include "common.h"

namespace {

constexpr int LN_MAXU = 4;          // 16-byte units per lane: rows of up to 64 * 4 * 4 = 1024 floats
constexpr int AT_D = 64;            // head dimension
constexpr int AT_T = 64;            // longest sequence of the short-sequence attention kernel
constexpr int POOL_L = 64;          // widest words_embs row (TEXT.MAX_LENGTH)

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

__global__ __launch_bounds__(256) void roberta_embed_ln_kernel(const int64_t* __restrict__ ids, const int32_t* __restrict__ lens,
                                                               const f32x4* __restrict__ word, const f32x4* __restrict__ pos,
                                                               const f32x4* __restrict__ type0, const f32x4* __restrict__ gamma,
                                                               const f32x4* __restrict__ beta, f32x4* __restrict__ out,
                                                               bf16x4* __restrict__ out16, int B, int T, int H, int64_t vocab, int npos,
                                                               int pad_idx, float eps) {
    const int lane = threadIdx.x & 63, H4 = H >> 2;
    const int64_t rows = (int64_t)B * T;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * 4) {
        const int b = (int)(row / T), t = (int)(row % T);
        const int len = min(max(lens[b], 0), T);
        const int64_t id = ids[row];
        const int p = t < len ? t + 1 + pad_idx : pad_idx;
        const bool ok = id >= 0 && id < vocab && p >= 0 && p < npos;       // the host wrapper validates; never read outside a table
        const f32x4* wr = word + (ok ? id : 0) * H4;
        const f32x4* pr = pos + (size_t)(ok ? p : 0) * H4;
        f32x4 v[LN_MAXU];
#pragma unroll
        for (int k = 0; k < LN_MAXU; ++k) {
            const int u = lane + 64 * k;
            v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (u < H4 && ok) v[k] = wr[u] + type0[u] + pr[u];
        }
        ln_row_store(v, lane, H4, H, gamma, beta, eps, out + row * H4, out16 ? out16 + row * H4 : nullptr);
    }
}

__global__ __launch_bounds__(256) void add_layernorm_kernel(const f32x4* __restrict__ x, const f32x4* __restrict__ bias,
                                                            const f32x4* __restrict__ res, const f32x4* __restrict__ gamma,
                                                            const f32x4* __restrict__ beta, f32x4* __restrict__ out,
                                                            bf16x4* __restrict__ out16, int64_t rows, int H, float eps) {
    const int lane = threadIdx.x & 63, H4 = H >> 2;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * 4) {
        f32x4 v[LN_MAXU];
#pragma unroll
        for (int k = 0; k < LN_MAXU; ++k) {
            const int u = lane + 64 * k;
            v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (u < H4) {
                v[k] = x[row * H4 + u];
                if (bias) v[k] += bias[u];
                if (res) v[k] += res[row * H4 + u];
            }
        }
        ln_row_store(v, lane, H4, H, gamma, beta, eps, out + row * H4, out16 ? out16 + row * H4 : nullptr);
    }
}

// one workgroup = one (sample, head); qkv rows are [Q (H) | K (H) | V (H)], head h in columns [64 h, 64 h + 64) of each
template <int ODT>
__global__ __launch_bounds__(256) void attention_short_kernel(const float* __restrict__ qkv, const int32_t* __restrict__ lens,
                                                              void* __restrict__ out, int T, int H) {
    // LDS sized by T, not by the longest sequence the kernel takes: at T = 20 a workgroup holds 15 KiB and eight of them share a CU
    extern __shared__ __attribute__((aligned(16))) float at_smem[];
    float (*q_s)[AT_D] = reinterpret_cast<float (*)[AT_D]>(at_smem);                          // [T][64]
    float (*v_s)[AT_D] = reinterpret_cast<float (*)[AT_D]>(at_smem + (size_t)T * AT_D);       // [T][64]
    float (*k_s)[AT_D + 1] = reinterpret_cast<float (*)[AT_D + 1]>(at_smem + (size_t)2 * T * AT_D);   // [T][65]: read with the key on the lane,
                                                                                              // odd row stride, no bank conflict
    const int b = blockIdx.x, head = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int len = min(max(lens[b], 0), T);
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
        if (r < len) {
            // scores: lane j holds key j
            float s = 0.f;
            if (lane < len) {
#pragma unroll
                for (int d = 0; d < AT_D; d += 4) {
                    const f32x4 q = *reinterpret_cast<const f32x4*>(&q_s[r][d]);
                    s += q[0] * k_s[lane][d] + q[1] * k_s[lane][d + 1] + q[2] * k_s[lane][d + 2] + q[3] * k_s[lane][d + 3];
                }
                s *= 0.125f;                                  // 1 / sqrt(64)
            }
            const float m = wave_max(lane < len ? s : -INFINITY);
            const float p = lane < len ? expf(s - m) : 0.f;   // padded keys: excluded
            const float l = wave_sum(p);
            // context: lane d holds channel d; p of key j comes out of lane j's register (j is wave-uniform)
            for (int j = 0; j < len; ++j)
                o += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, p), j)) * v_s[j][lane];
            o /= l;
        }
        // rows of padded queries: zero (they are dropped by the pooling tail)
        const size_t idx = ((size_t)b * T + r) * H + head * AT_D + lane;
        if (ODT == XMC_F32) reinterpret_cast<float*>(out)[idx] = o;
        else reinterpret_cast<xmc_h16*>(out)[idx] = (xmc_h16)o;
    }
}

template <int ODT>
__global__ __launch_bounds__(256) void bias_gelu_kernel(const float* __restrict__ x, const float* __restrict__ bias,
                                                        void* __restrict__ out, int64_t n8, int F8) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
        float v[8], bv[8];
        Vec8<XMC_F32>::load(x, (size_t)i, v);
        Vec8<XMC_F32>::load(bias, (size_t)(i % F8), bv);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float a = v[k] + bv[k];
            v[k] = 0.5f * a * (1.f + erff(a * 0.70710678118654752f));
        }
        Vec8<ODT>::store(out, (size_t)i, v);
    }
}

// one workgroup per sample: 64 channels at a time through an LDS tile (read [t][c], written [c][t])
__global__ __launch_bounds__(256) void sbert_pool_kernel(const float* __restrict__ hidden, const int32_t* __restrict__ lens,
                                                         float* __restrict__ words, float* __restrict__ sent,
                                                         uint8_t* __restrict__ mask, int T, int H, int L, int normalize) {
    __shared__ float tile[64][POOL_L + 1];
    __shared__ float mean_s[64 * LN_MAXU * 4];           // H <= 1024
    __shared__ float norm_s;
    const int b = blockIdx.x, tid = threadIdx.x, c = tid & 63, t0 = tid >> 6;
    const int len = min(max(lens[b], 0), T);
    for (int t = tid; t < L; t += 256) mask[(size_t)b * L + t] = t >= len ? 1 : 0;
    float sq = 0.f;
    for (int c0 = 0; c0 < H; c0 += 64) {
        for (int t = t0; t < L; t += 4) tile[c][t] = t < len ? hidden[((size_t)b * T + t) * H + c0 + c] : 0.f;
        __syncthreads();
        for (int i = tid; i < 64 * L; i += 256) words[((size_t)b * H + c0) * L + i] = tile[i / L][i % L];
        if (tid < 64) {
            float s = 0.f;
            for (int t = 0; t < len; ++t) s += tile[tid][t];
            s = len > 0 ? s / (float)len : 0.f;                              // words_pooling 'MEAN' (encoder.py:16-23): sum over valid tokens / their count
            mean_s[c0 + tid] = s;
            sq += s * s;
        }
        __syncthreads();
    }
    if (tid < 64) {
        sq = wave_sum(sq);
        if (tid == 0) norm_s = normalize ? 1.f / fmaxf(sqrtf(sq), 1e-12f) : 1.f;       // F.normalize(p=2, dim=1), eps 1e-12
    }
    __syncthreads();
    const float sc = norm_s;
    for (int i = tid; i < H; i += 256) sent[(size_t)b * H + i] = mean_s[i] * sc;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
inline unsigned row_grid(int64_t rows) { return (unsigned)((rows + 3) / 4 < 8192 ? (rows + 3) / 4 : 8192); }

}  // namespace

extern "C" int xmc_roberta_embed_ln(const int64_t* ids, const int32_t* lens, const float* word, const float* pos, const float* type0,
                                    const float* gamma, const float* beta, float* out, void* out16, int B, int T, int H, int64_t vocab,
                                    int npos, int pad_idx, float eps, void* stream) {
    if (!ids || !lens || !word || !pos || !type0 || !gamma || !beta || !out) return XMC_EINVAL;
    if (B < 1 || T < 1 || vocab < 1 || npos < 1 || pad_idx < 0 || H < 64 || H % 64 || H > 256 * LN_MAXU) return XMC_ESHAPE;
    if ((int64_t)T + 1 + pad_idx > npos) return XMC_ESHAPE;              // the last position id must be inside the table
    if (!aligned16(word) || !aligned16(pos) || !aligned16(type0) || !aligned16(gamma) || !aligned16(beta) || !aligned16(out) ||
        !aligned8(out16))
        return XMC_EALIGN;
    hipLaunchKernelGGL(roberta_embed_ln_kernel, dim3(row_grid((int64_t)B * T)), dim3(256), 0, (hipStream_t)stream, ids, lens,
                       reinterpret_cast<const f32x4*>(word), reinterpret_cast<const f32x4*>(pos), reinterpret_cast<const f32x4*>(type0),
                       reinterpret_cast<const f32x4*>(gamma), reinterpret_cast<const f32x4*>(beta), reinterpret_cast<f32x4*>(out),
                       reinterpret_cast<bf16x4*>(out16), B, T, H, vocab, npos, pad_idx, eps);
    XMC_LAUNCH_CHECK();
    return 0;
}

extern "C" int xmc_add_layernorm(const float* x, const float* bias, const float* res, const float* gamma, const float* beta, float* out,
                                 void* out16, int64_t rows, int H, float eps, void* stream) {
    if (!x || !gamma || !beta || !out) return XMC_EINVAL;
    if (rows < 1 || H < 64 || H % 64 || H > 256 * LN_MAXU) return XMC_ESHAPE;
    if (!aligned16(x) || !aligned16(bias) || !aligned16(res) || !aligned16(gamma) || !aligned16(beta) || !aligned16(out) ||
        !aligned8(out16))
        return XMC_EALIGN;
    hipLaunchKernelGGL(add_layernorm_kernel, dim3(row_grid(rows)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const f32x4*>(x), reinterpret_cast<const f32x4*>(bias), reinterpret_cast<const f32x4*>(res),
                       reinterpret_cast<const f32x4*>(gamma), reinterpret_cast<const f32x4*>(beta), reinterpret_cast<f32x4*>(out),
                       reinterpret_cast<bf16x4*>(out16), rows, H, eps);
    XMC_LAUNCH_CHECK();
    return 0;
}

extern "C" int xmc_attention_short(const float* qkv, const int32_t* lens, void* out, int B, int T, int heads, int head_dim, int out_dtype,
                                   void* stream) {
    if (!qkv || !lens || !out || (out_dtype != XMC_BF16 && out_dtype != XMC_F32)) return XMC_EINVAL;
    if (B < 1 || heads < 1 || heads > 65535 || T < 1 || T > AT_T || head_dim != AT_D) return XMC_ESHAPE;    // other shapes are not built
    if (!aligned16(qkv)) return XMC_EALIGN;
    const int H = heads * AT_D;
    dim3 grid((unsigned)B, (unsigned)heads), blk(256);
    const size_t lds = (size_t)T * (3 * AT_D + 1) * sizeof(float);            // <= 49408 bytes at T = 64
    if (out_dtype == XMC_F32)
        hipLaunchKernelGGL(attention_short_kernel<XMC_F32>, grid, blk, lds, (hipStream_t)stream, qkv, lens, out, T, H);
    else
        hipLaunchKernelGGL(attention_short_kernel<XMC_BF16>, grid, blk, lds, (hipStream_t)stream, qkv, lens, out, T, H);
    XMC_LAUNCH_CHECK();
    return 0;
}

extern "C" int xmc_bias_gelu(const float* x, const float* bias, void* out, int64_t rows, int F, int out_dtype, void* stream) {
    if (!x || !bias || !out || (out_dtype != XMC_BF16 && out_dtype != XMC_F32)) return XMC_EINVAL;
    if (rows < 1 || F < 8) return XMC_ESHAPE;
    if (F % 8 || !aligned16(x) || !aligned16(bias) || !aligned16(out)) return XMC_EALIGN;
    const int64_t n8 = rows * (F / 8);
    const unsigned grid = (unsigned)((n8 + 255) / 256 < 16384 ? (n8 + 255) / 256 : 16384);
    if (out_dtype == XMC_F32)
        hipLaunchKernelGGL(bias_gelu_kernel<XMC_F32>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, bias, out, n8, F / 8);
    else
        hipLaunchKernelGGL(bias_gelu_kernel<XMC_BF16>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, bias, out, n8, F / 8);
    XMC_LAUNCH_CHECK();
    return 0;
}

extern "C" int xmc_sbert_pool(const float* hidden, const int32_t* lens, float* words, float* sent, uint8_t* mask, int B, int T, int H,
                              int L, int normalize, void* stream) {
    if (!hidden || !lens || !words || !sent || !mask) return XMC_EINVAL;
    if (B < 1 || T < 1 || T > L || L > POOL_L || H < 64 || H % 64 || H > 256 * LN_MAXU) return XMC_ESHAPE;
    hipLaunchKernelGGL(sbert_pool_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, hidden, lens, words, sent, mask, T, H, L,
                       normalize);
    XMC_LAUNCH_CHECK();
    return 0;
}
