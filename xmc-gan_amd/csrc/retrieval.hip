// R-precision (xmc_gan_amd/rprecision.py): for every image, the cosine between its code and the codes of K candidate captions, and how many of
// the K - 1 others beat the image's own caption (candidate 0).  The reference has no such evaluation; this is AttnGAN's protocol.
//
//   One wave per image (4 per workgroup).  The image row sits in registers as up to four 16-byte units per lane (unit u = lane + 64 j, so a
//   wave's load of a row is contiguous); D <= 1024.  The wave walks its image's candidate list: the index is one uniform load, the caption row
//   is fetched with 16-byte loads straight from `txt` -- the [N,K,D] gather exists nowhere -- and dot and |txt|^2 are reduced over the wave by
//   the xor butterfly of common.h (a fixed order; every lane ends with the same bits).  Candidates go four at a time so that four rows'
//   loads are in flight before the first reduction.  No atomics, no LDS: the same inputs give the same bytes.
//   An index outside [0, M) is the caller's error (the Python wrapper refuses it on the host); such a row is not read and scores NaN.
#include "common.h"

namespace {
constexpr int NT = 256, WAVES = NT / 64, KU = 4;          // candidates per round

template <int U>
__device__ __forceinline__ void row_products(const f32x4 (&a)[U], const float* __restrict__ row, int units, int lane, float& dot, float& nn) {
    const f32x4* __restrict__ r4 = reinterpret_cast<const f32x4*>(row);
    dot = 0.f; nn = 0.f;
#pragma unroll
    for (int j = 0; j < U; ++j) {
        const int u = lane + 64 * j;
        if (u < units) {
            const f32x4 t = r4[u];
#pragma unroll
            for (int e = 0; e < 4; ++e) { dot = fmaf(a[j][e], t[e], dot); nn = fmaf(t[e], t[e], nn); }
        }
    }
}

template <int U>
__global__ void __launch_bounds__(NT) rprecision_kernel(const float* __restrict__ img, const float* __restrict__ txt, const int32_t* __restrict__ cand,
                                                       int32_t* __restrict__ rank, float* __restrict__ score, int N, int M, int K, int D) {
    const int lane = threadIdx.x & 63, units = D >> 2;
    const int n = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (n >= N) return;                                    // (whole waves; nothing below synchronises a workgroup)
    f32x4 a[U];
    float na = 0.f;
#pragma unroll
    for (int j = 0; j < U; ++j) {
        const int u = lane + 64 * j;
        a[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (u < units) a[j] = reinterpret_cast<const f32x4*>(img + (size_t)n * D)[u];
#pragma unroll
        for (int e = 0; e < 4; ++e) na = fmaf(a[j][e], a[j][e], na);
    }
    const float norm_a = sqrtf(wave_sum(na));
    const int32_t* __restrict__ cn = cand + (size_t)n * K;
    float s0 = 0.f;
    int beat = 0;
    for (int k0 = 0; k0 < K; k0 += KU) {
        float dot[KU], nn[KU];
        bool ok[KU];
#pragma unroll
        for (int i = 0; i < KU; ++i) {
            const int k = k0 + i;
            const int c = k < K ? cn[k] : -1;
            ok[i] = (unsigned)c < (unsigned)M;
            dot[i] = 0.f; nn[i] = 0.f;
            if (ok[i]) row_products<U>(a, txt + (size_t)c * D, units, lane, dot[i], nn[i]);
        }
#pragma unroll
        for (int i = 0; i < KU; ++i) { dot[i] = wave_sum(dot[i]); nn[i] = wave_sum(nn[i]); }
#pragma unroll
        for (int i = 0; i < KU; ++i) {
            const int k = k0 + i;
            if (k >= K) break;
            const float s = ok[i] ? dot[i] / fmaxf(norm_a * sqrtf(nn[i]), 1e-8f) : __builtin_nanf("");
            if (score && lane == 0) score[(size_t)n * K + k] = s;
            if (k == 0) s0 = s;
            else if (s > s0) ++beat;
        }
    }
    if (lane == 0) rank[n] = (s0 != s0) ? K : beat;
}
}  // namespace

extern "C" int xmc_rprecision(const float* img, const float* txt, const int32_t* cand, int32_t* rank, float* score, int N, int M, int K, int D,
                              void* stream) {
    if (!img || !txt || !cand || !rank || N < 1 || M < 1 || K < 1) return XMC_EINVAL;
    if (D < 4 || D % 4 != 0 || D > 1024) return XMC_ESHAPE;
    if ((reinterpret_cast<uintptr_t>(img) | reinterpret_cast<uintptr_t>(txt)) & 15) return XMC_EALIGN;
    if ((reinterpret_cast<uintptr_t>(cand) | reinterpret_cast<uintptr_t>(rank) | reinterpret_cast<uintptr_t>(score)) & 3) return XMC_EALIGN;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((N + WAVES - 1) / WAVES), block(NT);
    const int U = (D / 4 + 63) / 64;
#define XMC_RP_GO(U_) hipLaunchKernelGGL((rprecision_kernel<U_>), grid, block, 0, st, img, txt, cand, rank, score, N, M, K, D)
    if (U == 1) XMC_RP_GO(1); else if (U == 2) XMC_RP_GO(2); else if (U == 3) XMC_RP_GO(3); else XMC_RP_GO(4);
#undef XMC_RP_GO
    xmc_note_kernel("rprecision_kernel<%d>", U);
    XMC_LAUNCH_CHECK();
    return 0;
}
