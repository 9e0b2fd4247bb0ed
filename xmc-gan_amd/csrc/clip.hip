// CLIPScore (xmc_gan_amd/clip.py): what the two CLIP towers need besides the f32 GEMMs of the 1x1 convolution path and the
// LayerNorm / short-sequence attention / erf-GELU entry points of transformer.hip.  Forward only, f32 in every build, no atomics anywhere:
// every output element has one writer and a fixed summation order, so the same inputs give the same bytes.
//
//   xmc_clip_resize_h_u8   Pillow's antialiased resize of an 8-bit image along x, bit for bit: int32 coefficients (22 fraction bits) and
//   xmc_clip_resize_v_u8   bounds from the host, clip8((2^21 + sum pixel * k) >> 22); then the same along y, writing either the uint8
//                          image or CLIP's input: centre crop, per-channel normalisation table, patch-major f32 rows
//   xmc_attention_causal   softmax(Q K^T / sqrt(64)) V over keys j <= i per (sample, head), T <= 64 (encoder_kernels.h: attention_kernel<f32, causal>)
//   xmc_bias_quick_gelu    v = x + bias; v * sigmoid(1.702 v), streaming in 8-element units (encoder_kernels.h: bias_act_kernel)
//   xmc_clip_vision_embed  [class + pos[0] | patch[p] + pos[1 + p]] then LayerNorm: one wave per token row
//   xmc_clip_text_embed    token[ids] + pos[t]: one wave per token row
//   xmc_clip_pool_ln       LayerNorm of one row per sample, picked by an index
//   xmc_clip_cosine        per image, the cosine of its feature row and its caption's: one wave per image
#include "encoder_kernels.h"

namespace {

constexpr int RS_NT = 256;

__device__ __forceinline__ uint8_t clip8(int32_t acc) {
    const int32_t v = acc >> 22;    // arithmetic shift: a negative sum stays negative and clamps to 0 (Pillow's clip8)
    return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// one thread per output pixel (n, y, xx): its window [xmin, xmin + cnt) of the source row, three channels
__global__ __launch_bounds__(RS_NT) void clip_resize_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                              const int32_t* __restrict__ bounds, const int32_t* __restrict__ coeffs,
                                                              int64_t total, int W, int OW, int ksize) {
    for (int64_t i = (int64_t)blockIdx.x * RS_NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * RS_NT) {
        const int xx = (int)(i % OW);
        const int64_t row = i / OW;                                    // n * H + y
        const int xmin = min(max(bounds[2 * xx], 0), W - 1);           // the host validates; never read outside the row
        const int cnt = min(min(max(bounds[2 * xx + 1], 0), ksize), W - xmin);
        const int32_t* k = coeffs + (size_t)xx * ksize;
        const uint8_t* p = src + ((size_t)row * W + xmin) * 3;
        int32_t a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
        for (int x = 0; x < cnt; ++x) {
            const int32_t kx = k[x];
            a0 += (int32_t)p[3 * x] * kx;
            a1 += (int32_t)p[3 * x + 1] * kx;
            a2 += (int32_t)p[3 * x + 2] * kx;
        }
        uint8_t* o = dst + (size_t)i * 3;
        o[0] = clip8(a0), o[1] = clip8(a1), o[2] = clip8(a2);
    }
}

// one thread per output pixel; MODE 0: the uint8 image [N,OH,OW,3]; MODE 1: the S x S centre crop, normalised through `lut` [3][256] and
// written patch-major: row (n, y / P, x / P), column c P^2 + (y % P) P + x % P  (the flatten order of patch_embedding.weight)
template <int MODE>
__global__ __launch_bounds__(RS_NT) void clip_resize_v_kernel(const uint8_t* __restrict__ src, void* __restrict__ dst,
                                                              const int32_t* __restrict__ bounds, const int32_t* __restrict__ coeffs,
                                                              const float* __restrict__ lut, int64_t total, int H, int W, int OH, int ksize,
                                                              int S, int P, int top, int left) {
    const int RW = MODE == 0 ? W : S, RH = MODE == 0 ? OH : S;         // the region this launch writes
    for (int64_t i = (int64_t)blockIdx.x * RS_NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * RS_NT) {
        const int rx = (int)(i % RW), ry = (int)((i / RW) % RH);
        const int64_t n = i / ((int64_t)RW * RH);
        const int x = MODE == 0 ? rx : rx + left, yy = MODE == 0 ? ry : ry + top;
        const int ymin = min(max(bounds[2 * yy], 0), H - 1);
        const int cnt = min(min(max(bounds[2 * yy + 1], 0), ksize), H - ymin);
        const int32_t* k = coeffs + (size_t)yy * ksize;
        const uint8_t* p = src + (((size_t)n * H + ymin) * W + x) * 3;
        const size_t rs = (size_t)W * 3;
        int32_t a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
        for (int y = 0; y < cnt; ++y) {
            const int32_t ky = k[y];
            a0 += (int32_t)p[y * rs] * ky;
            a1 += (int32_t)p[y * rs + 1] * ky;
            a2 += (int32_t)p[y * rs + 2] * ky;
        }
        if (MODE == 0) {
            uint8_t* o = reinterpret_cast<uint8_t*>(dst) + (size_t)i * 3;
            o[0] = clip8(a0), o[1] = clip8(a1), o[2] = clip8(a2);
        } else {
            const int G = S / P, PP = P * P;
            float* o = reinterpret_cast<float*>(dst) + (((size_t)n * G + ry / P) * G + rx / P) * 3 * PP + (ry % P) * P + rx % P;
            o[0] = lut[clip8(a0)];
            o[PP] = lut[256 + clip8(a1)];
            o[2 * PP] = lut[512 + clip8(a2)];
        }
    }
}

__global__ __launch_bounds__(256) void clip_vision_embed_kernel(const f32x4* __restrict__ patch, const f32x4* __restrict__ cls,
                                                                const f32x4* __restrict__ pos, const f32x4* __restrict__ gamma,
                                                                const f32x4* __restrict__ beta, f32x4* __restrict__ out, int64_t rows,
                                                                int GG, int H, float eps) {
    const int lane = threadIdx.x & 63, H4 = H >> 2, T = GG + 1;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * 4) {
        const int64_t n = row / T;
        const int t = (int)(row % T);
        const f32x4* a = t == 0 ? cls : patch + (n * GG + (t - 1)) * H4;
        const f32x4* p = pos + (size_t)t * H4;
        f32x4 v[LN_MAXU];
#pragma unroll
        for (int k = 0; k < LN_MAXU; ++k) {
            const int u = lane + 64 * k;
            v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (u < H4) v[k] = a[u] + p[u];
        }
        ln_row_store(v, lane, H4, H, gamma, beta, eps, out + row * H4, nullptr);
    }
}

__global__ __launch_bounds__(256) void clip_text_embed_kernel(const int64_t* __restrict__ ids, const f32x4* __restrict__ tok,
                                                              const f32x4* __restrict__ pos, f32x4* __restrict__ out, int64_t rows, int T,
                                                              int H, int64_t vocab) {
    const int lane = threadIdx.x & 63, H4 = H >> 2;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * 4) {
        const int t = (int)(row % T);
        const int64_t id = ids[row];
        const bool ok = id >= 0 && id < vocab;                 // the host wrapper validates; never read outside the table
        const f32x4* a = tok + (ok ? id : 0) * H4;
        const f32x4* p = pos + (size_t)t * H4;
        for (int u = lane; u < H4; u += 64) out[row * H4 + u] = ok ? a[u] + p[u] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

__global__ __launch_bounds__(256) void clip_pool_ln_kernel(const f32x4* __restrict__ x, const int32_t* __restrict__ index,
                                                           const f32x4* __restrict__ gamma, const f32x4* __restrict__ beta,
                                                           f32x4* __restrict__ out, int B, int T, int H, float eps) {
    const int lane = threadIdx.x & 63, H4 = H >> 2;
    for (int b = blockIdx.x * 4 + (threadIdx.x >> 6); b < B; b += gridDim.x * 4) {
        const int t = min(max(index[b], 0), T - 1);
        const f32x4* r = x + ((size_t)b * T + t) * H4;
        f32x4 v[LN_MAXU];
#pragma unroll
        for (int k = 0; k < LN_MAXU; ++k) {
            const int u = lane + 64 * k;
            v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (u < H4) v[k] = r[u];
        }
        ln_row_store(v, lane, H4, H, gamma, beta, eps, out + (size_t)b * H4, nullptr);
    }
}

// one wave per image: lane l sums elements l, l + 64, ... in order, then the butterfly: a fixed order
__global__ __launch_bounds__(256) void clip_cosine_kernel(const float* __restrict__ img, const float* __restrict__ txt,
                                                          const int32_t* __restrict__ cap, float* __restrict__ out, int N, int M, int D) {
    const int lane = threadIdx.x & 63;
    for (int n = blockIdx.x * 4 + (threadIdx.x >> 6); n < N; n += gridDim.x * 4) {
        const int m = min(max(cap ? cap[n] : n, 0), M - 1);
        const float* a = img + (size_t)n * D;
        const float* b = txt + (size_t)m * D;
        float ab = 0.f, aa = 0.f, bb = 0.f;
        for (int d = lane; d < D; d += 64) {
            const float x = a[d], y = b[d];
            ab += x * y, aa += x * x, bb += y * y;
        }
        ab = wave_sum(ab), aa = wave_sum(aa), bb = wave_sum(bb);
        if (lane == 0) out[n] = ab / fmaxf(sqrtf(aa) * sqrtf(bb), 1e-30f);
    }
}

inline unsigned px_grid(int64_t n) { return (unsigned)((n + RS_NT - 1) / RS_NT < 16384 ? (n + RS_NT - 1) / RS_NT : 16384); }

}  // namespace

extern "C" int xmc_clip_resize_h_u8(const uint8_t* src, uint8_t* dst, const int32_t* bounds, const int32_t* coeffs, int N, int H, int W,
                                    int OW, int ksize, void* stream) {
    if (!src || !dst || !bounds || !coeffs) return XMC_EINVAL;
    if (N < 1 || H < 1 || W < 1 || OW < 1 || ksize < 1 || ksize > 4096) return XMC_ESHAPE;
    if ((int64_t)H * W > (int64_t)1 << 28 || (int64_t)H * OW > (int64_t)1 << 28) return XMC_ESHAPE;
    if (!aligned4(bounds) || !aligned4(coeffs)) return XMC_EALIGN;
    const int64_t total = (int64_t)N * H * OW;
    hipLaunchKernelGGL(clip_resize_h_kernel, dim3(px_grid(total)), dim3(RS_NT), 0, (hipStream_t)stream, src, dst, bounds, coeffs, total, W,
                       OW, ksize);
    xmc_note_kernel("clip_resize_h_kernel");
    XMC_LAUNCH_CHECK();
    return 0;
}

extern "C" int xmc_clip_resize_v_u8(const uint8_t* src, void* dst, const int32_t* bounds, const int32_t* coeffs, const float* lut, int N,
                                    int H, int W, int OH, int ksize, int mode, int S, int P, int top, int left, void* stream) {
    if (!src || !dst || !bounds || !coeffs || (mode != 0 && mode != 1) || (mode == 1 && !lut)) return XMC_EINVAL;
    if (N < 1 || H < 1 || W < 1 || OH < 1 || ksize < 1 || ksize > 4096) return XMC_ESHAPE;
    if ((int64_t)H * W > (int64_t)1 << 28 || (int64_t)OH * W > (int64_t)1 << 28) return XMC_ESHAPE;
    if (mode == 1 && (S < 1 || P < 1 || S % P || top < 0 || left < 0 || (int64_t)top + S > OH || (int64_t)left + S > W)) return XMC_ESHAPE;
    if (!aligned4(bounds) || !aligned4(coeffs) || (mode == 1 && (!aligned4(lut) || !aligned4(dst)))) return XMC_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    if (mode == 0) {
        const int64_t total = (int64_t)N * OH * W;
        hipLaunchKernelGGL(clip_resize_v_kernel<0>, dim3(px_grid(total)), dim3(RS_NT), 0, st, src, dst, bounds, coeffs, lut, total, H, W,
                           OH, ksize, 0, 1, 0, 0);
    } else {
        const int64_t total = (int64_t)N * S * S;
        hipLaunchKernelGGL(clip_resize_v_kernel<1>, dim3(px_grid(total)), dim3(RS_NT), 0, st, src, dst, bounds, coeffs, lut, total, H, W,
                           OH, ksize, S, P, top, left);
    }
    xmc_note_kernel("clip_resize_v_kernel<%d>", mode);
    XMC_LAUNCH_CHECK();
    return 0;
}

extern "C" int xmc_attention_causal(const float* qkv, float* out, int B, int T, int heads, int head_dim, void* stream) {
    if (!qkv || !out) return XMC_EINVAL;
    if (B < 1 || heads < 1 || heads > 65535 || T < 1 || T > AT_T || head_dim != AT_D) return XMC_ESHAPE;    // other shapes are not built
    if (!aligned16(qkv) || !aligned4(out)) return XMC_EALIGN;
    const size_t lds = (size_t)T * (3 * AT_D + 1) * sizeof(float);            // <= 49408 bytes at T = 64
    hipLaunchKernelGGL((attention_kernel<XMC_F32, true>), dim3((unsigned)B, (unsigned)heads), dim3(256), lds, (hipStream_t)stream, qkv,
                       (const int32_t*)nullptr, (void*)out, T, heads * AT_D);
    xmc_note_kernel("attention_kernel<f32,true>");
    XMC_LAUNCH_CHECK();
    return 0;
}

extern "C" int xmc_bias_quick_gelu(const float* x, const float* bias, float* out, int64_t rows, int F, void* stream) {
    if (!x || !bias || !out) return XMC_EINVAL;
    if (rows < 1 || F < 8) return XMC_ESHAPE;
    if (F % 8 || !aligned16(x) || !aligned16(bias) || !aligned16(out)) return XMC_EALIGN;
    const int64_t n8 = rows * (F / 8);
    const unsigned grid = (unsigned)((n8 + 255) / 256 < 16384 ? (n8 + 255) / 256 : 16384);
    hipLaunchKernelGGL((bias_act_kernel<XMC_F32, ACT_QUICK_GELU>), dim3(grid), dim3(256), 0, (hipStream_t)stream, x, bias, (void*)out, n8,
                       F / 8);
    xmc_note_kernel("bias_act_kernel<f32,%d>", ACT_QUICK_GELU);
    XMC_LAUNCH_CHECK();
    return 0;
}

extern "C" int xmc_clip_vision_embed(const float* patch, const float* cls, const float* pos, const float* gamma, const float* beta,
                                     float* out, int N, int GG, int H, float eps, void* stream) {
    if (!patch || !cls || !pos || !gamma || !beta || !out) return XMC_EINVAL;
    if (N < 1 || GG < 1 || GG > 65535 || !ln_width(H)) return XMC_ESHAPE;
    if (!aligned16(patch) || !aligned16(cls) || !aligned16(pos) || !aligned16(gamma) || !aligned16(beta) || !aligned16(out)) return XMC_EALIGN;
    const int64_t rows = (int64_t)N * (GG + 1);
    hipLaunchKernelGGL(clip_vision_embed_kernel, dim3(row_grid(rows)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const f32x4*>(patch), reinterpret_cast<const f32x4*>(cls), reinterpret_cast<const f32x4*>(pos),
                       reinterpret_cast<const f32x4*>(gamma), reinterpret_cast<const f32x4*>(beta), reinterpret_cast<f32x4*>(out), rows, GG,
                       H, eps);
    xmc_note_kernel("clip_vision_embed_kernel");
    XMC_LAUNCH_CHECK();
    return 0;
}

extern "C" int xmc_clip_text_embed(const int64_t* ids, const float* tok, const float* pos, float* out, int B, int T, int H, int64_t vocab,
                                   int npos, void* stream) {
    if (!ids || !tok || !pos || !out) return XMC_EINVAL;
    if (B < 1 || T < 1 || vocab < 1 || npos < 1 || T > npos || !ln_width(H)) return XMC_ESHAPE;
    if ((reinterpret_cast<uintptr_t>(ids) & 7) || !aligned16(tok) || !aligned16(pos) || !aligned16(out)) return XMC_EALIGN;
    const int64_t rows = (int64_t)B * T;
    hipLaunchKernelGGL(clip_text_embed_kernel, dim3(row_grid(rows)), dim3(256), 0, (hipStream_t)stream, ids,
                       reinterpret_cast<const f32x4*>(tok), reinterpret_cast<const f32x4*>(pos), reinterpret_cast<f32x4*>(out), rows, T, H,
                       vocab);
    xmc_note_kernel("clip_text_embed_kernel");
    XMC_LAUNCH_CHECK();
    return 0;
}

extern "C" int xmc_clip_pool_ln(const float* x, const int32_t* index, const float* gamma, const float* beta, float* out, int B, int T,
                                int H, float eps, void* stream) {
    if (!x || !index || !gamma || !beta || !out) return XMC_EINVAL;
    if (B < 1 || T < 1 || !ln_width(H)) return XMC_ESHAPE;
    if (!aligned16(x) || !aligned4(index) || !aligned16(gamma) || !aligned16(beta) || !aligned16(out)) return XMC_EALIGN;
    hipLaunchKernelGGL(clip_pool_ln_kernel, dim3(row_grid(B)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const f32x4*>(x), index,
                       reinterpret_cast<const f32x4*>(gamma), reinterpret_cast<const f32x4*>(beta), reinterpret_cast<f32x4*>(out), B, T, H,
                       eps);
    xmc_note_kernel("clip_pool_ln_kernel");
    XMC_LAUNCH_CHECK();
    return 0;
}

extern "C" int xmc_clip_cosine(const float* img, const float* txt, const int32_t* caption_of_image, float* out, int N, int M, int D,
                               void* stream) {
    if (!img || !txt || !out) return XMC_EINVAL;
    if (N < 1 || M < 1 || D < 1 || (!caption_of_image && N > M)) return XMC_ESHAPE;
    if (!aligned4(img) || !aligned4(txt) || !aligned4(caption_of_image) || !aligned4(out)) return XMC_EALIGN;
    hipLaunchKernelGGL(clip_cosine_kernel, dim3(row_grid(N)), dim3(256), 0, (hipStream_t)stream, img, txt, caption_of_image, out, N, M, D);
    xmc_note_kernel("clip_cosine_kernel");
    XMC_LAUNCH_CHECK();
    return 0;
}
