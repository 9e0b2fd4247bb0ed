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
// The LayerNorm row, the attention kernel and the bias + activation kernel are encoder_kernels.h's, shared with clip.hip.
#include "encoder_kernels.h"

namespace {

constexpr int POOL_L = 64;          // widest words_embs row (TEXT.MAX_LENGTH)

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
    xmc_note_kernel("roberta_embed_ln_kernel");
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
    xmc_note_kernel("add_layernorm_kernel");
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
        hipLaunchKernelGGL((attention_kernel<XMC_F32, false>), grid, blk, lds, (hipStream_t)stream, qkv, lens, out, T, H);
    else
        hipLaunchKernelGGL((attention_kernel<XMC_BF16, false>), grid, blk, lds, (hipStream_t)stream, qkv, lens, out, T, H);
    xmc_note_kernel("attention_kernel<%s,false>", out_dtype == XMC_BF16 ? "h16" : "f32");
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
        hipLaunchKernelGGL((bias_act_kernel<XMC_F32, ACT_GELU>), dim3(grid), dim3(256), 0, (hipStream_t)stream, x, bias, out, n8, F / 8);
    else
        hipLaunchKernelGGL((bias_act_kernel<XMC_BF16, ACT_GELU>), dim3(grid), dim3(256), 0, (hipStream_t)stream, x, bias, out, n8, F / 8);
    xmc_note_kernel("bias_act_kernel<%s,%d>", out_dtype == XMC_BF16 ? "h16" : "f32", ACT_GELU);
    XMC_LAUNCH_CHECK();
    return 0;
}

extern "C" int xmc_sbert_pool(const float* hidden, const int32_t* lens, float* words, float* sent, uint8_t* mask, int B, int T, int H,
                              int L, int normalize, void* stream) {
    if (!hidden || !lens || !words || !sent || !mask) return XMC_EINVAL;
    if (B < 1 || T < 1 || T > L || L > POOL_L || H < 64 || H % 64 || H > 256 * LN_MAXU) return XMC_ESHAPE;
    hipLaunchKernelGGL(sbert_pool_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, hidden, lens, words, sent, mask, T, H, L,
                       normalize);
    xmc_note_kernel("sbert_pool_kernel");
    XMC_LAUNCH_CHECK();
    return 0;
}
