// Differentiable augmentation of the discriminator's input images (Zhao et al., "Differentiable Augmentation for Data-Efficient GAN
// Training"; not in the reference): brightness, saturation, contrast, integer translation with zero fill, cutout -- one affine map
// y = A x + (b-term) per image, in the engine's [N,H,W,8] image layout (C real channels, zero padding after them).
//
// Per image n one f32 row P[n] = (b, s, c, tx, ty, cy, cx, 0), the geometric entries integers stored as floats; with u = x + b,
// p = mean_k u, v = s u + (1 - s) p, m = mean_{q,k} v = mean(x) + b, w = c v + (1 - c) m, output pixel (i, j) is w at (i + ty, j + tx) when
// that source is inside the image and (i, j) is outside the square [cy, cy + cut) x [cx, cx + cut), else 0.  The rows live in device memory
// and are read by the kernels, so a captured graph sees every new draw.
//
// Two passes per direction, each one 16-byte load per pixel in the 16-bit formats:
//   sums   per-image partial sums (forward: of x; transposed: of the dy a source pixel receives), one partial per workgroup, no atomics:
//          XMC_DIFFAUG_PARTS slots per image of which the first diffaug_parts(H*W) are written.  Skipped by a policy without colour.
//   apply  forward (gather x at the shifted source, colour, mask) or transposed (gather dy at the shifted destination, mask, A^T of the
//          colour part); adds the partials of its image in a fixed order first, so the result does not depend on scheduling.
// All arithmetic is f32; `s*u + (1-s)*p` and `c*v + (1-c)*m` are written in exactly these forms, which makes (b, s, c) = (0, 1, 1) with no
// shift and no cutout a bit-exact copy in every storage format.
#include "common.h"

namespace {
constexpr int NT = 256;
constexpr int PIX_PER_THREAD = 4;

inline int diffaug_parts(int HW) {
    const int p = (HW + NT * PIX_PER_THREAD - 1) / (NT * PIX_PER_THREAD);
    return p < XMC_DIFFAUG_PARTS ? p : XMC_DIFFAUG_PARTS;
}

struct Row {
    float b, s, c;
    int tx, ty, cy, cx;
};
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// (shifts beyond the frame and squares far outside it are clamped to "just outside": the same result, and no overflow in i + ty)
__device__ __forceinline__ Row load_row(const float* __restrict__ P, int n, int H, int W) {
    const f32x4* p = reinterpret_cast<const f32x4*>(P + (size_t)n * 8);
    const f32x4 a = p[0], g = p[1];
    Row r;
    r.b = a[0]; r.s = a[1]; r.c = a[2];
    r.tx = clampi((int)a[3], -W, W);
    r.ty = clampi((int)g[0], -H, H);
    r.cy = clampi((int)g[1], -(1 << 20), 1 << 20);
    r.cx = clampi((int)g[2], -(1 << 20), 1 << 20);
    return r;
}
__device__ __forceinline__ bool in_cut(const Row& r, int i, int j, int cut) {
    return i >= r.cy && i < r.cy + cut && j >= r.cx && j < r.cx + cut;
}

// the first C (<= 8) channels of pixel `pix8` as floats; the others are not read where the format allows
template <int DT> __device__ __forceinline__ void load_px(const void* p, size_t pix8, int C, float (&v)[8]);
template <> __device__ __forceinline__ void load_px<XMC_BF16>(const void* p, size_t pix8, int, float (&v)[8]) {
    Vec8<XMC_BF16>::load(p, pix8, v);
}
template <> __device__ __forceinline__ void load_px<XMC_F32>(const void* p, size_t pix8, int C, float (&v)[8]) {
    const f32x4* q = reinterpret_cast<const f32x4*>(p) + pix8 * 2;
    const f32x4 a = q[0];
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = a[k]; v[4 + k] = 0.f; }
    if (C > 4) {
        const f32x4 b = q[1];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[4 + k] = b[k];
    }
}

// sum over the workgroup; valid in thread 0
__device__ __forceinline__ float block_sum(float v) {
    __shared__ float red[NT / 64];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) t += red[w];
    }
    return t;
}

// grid (parts, N).  TR = false: partial sums of x over pixels and channels < C.  TR = true: of dy over the output pixels that are outside
// the cutout square and whose source lies inside the image (the pixels whose dy reaches some x).
template <int DT, bool TR>
__global__ void __launch_bounds__(NT) diffaug_sums_kernel(const void* __restrict__ x, const float* __restrict__ P, float* __restrict__ parts,
                                                         int H, int W, int C, int cut) {
    const int n = blockIdx.y, HW = H * W;
    Row r;
    if (TR) r = load_row(P, n, H, W);
    float acc = 0.f;
    for (int pix = blockIdx.x * NT + threadIdx.x; pix < HW; pix += gridDim.x * NT) {
        if (TR) {
            const int i = pix / W, j = pix - i * W, si = i + r.ty, sj = j + r.tx;
            if (si < 0 || si >= H || sj < 0 || sj >= W || in_cut(r, i, j, cut)) continue;
        }
        float v[8];
        load_px<DT>(x, (size_t)n * HW + pix, C, v);
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < C) acc += v[k];
    }
    const float t = block_sum(acc);
    if (threadIdx.x == 0) parts[(size_t)n * XMC_DIFFAUG_PARTS + blockIdx.x] = t;
}

// grid (blocks per image, N), one pixel per lane and trip.  `parts` == NULL: a policy without colour (c == 1 in every row, so the image
// mean has weight 0): nothing is read through it.  LIN: the linear part only (b ignored).
template <int DT, bool TR>
__global__ void __launch_bounds__(NT) diffaug_apply_kernel(const void* __restrict__ x, const float* __restrict__ P, const float* __restrict__ parts,
                                                          void* __restrict__ y, int H, int W, int C, int cut, int nparts, int lin) {
    __shared__ float total;
    const int n = blockIdx.y, HW = H * W;
    const Row r = load_row(P, n, H, W);
    float sum = 0.f;
    if (parts) {                      // the image's partials, added in one fixed order by the first wave
        if (threadIdx.x < 64) {
            const float t = wave_sum((int)threadIdx.x < nparts ? parts[(size_t)n * XMC_DIFFAUG_PARTS + threadIdx.x] : 0.f);
            if (threadIdx.x == 0) total = t;
        }
        __syncthreads();
        sum = total;
    }
    const float b = (lin || TR) ? 0.f : r.b, s = r.s, c = r.c;
    const float invC = 1.f / (float)C, mean = sum / (float)(C * HW);
    for (int pix = blockIdx.x * NT + threadIdx.x; pix < HW; pix += gridDim.x * NT) {
        const int i = pix / W, j = pix - i * W;
        // forward: output (i, j) reads x at (i + ty, j + tx) and is masked by its own position; transposed: source (i, j) reads dy at
        // (i - ty, j - tx), masked by THAT position
        const int si = TR ? i - r.ty : i + r.ty, sj = TR ? j - r.tx : j + r.tx;
        const bool live = si >= 0 && si < H && sj >= 0 && sj < W && !(TR ? in_cut(r, si, sj, cut) : in_cut(r, i, j, cut));
        float v[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = o[k] = 0.f;
        if (live) load_px<DT>(x, (size_t)n * HW + (size_t)si * W + sj, C, v);
        if (!TR) {
            if (live) {
                const float m = mean + b;
                float ps = 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (k < C) { v[k] = v[k] + b; ps += v[k]; }
                const float p = invC * ps;
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (k < C) {
                        const float vv = s * v[k] + (1.f - s) * p;
                        o[k] = c * vv + (1.f - c) * m;
                    }
            }
        } else {                      // a source shifted out of the frame still receives the mean's share
            float ds = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (k < C) { v[k] = c * v[k] + (1.f - c) * mean; ds += v[k]; }
            const float p = invC * ds;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (k < C) o[k] = s * v[k] + (1.f - s) * p;
        }
        Vec8<DT>::store(y, (size_t)n * HW + pix, o);
    }
}

int check_args(const void* x, const float* params, int N, int H, int W, int C, int cut, int dtype) {
    if (!x || !params || N < 1 || H < 1 || W < 1) return XMC_EINVAL;
    if (C > 8 || C < 1 || cut < 0 || (dtype != XMC_BF16 && dtype != XMC_F32)) return XMC_ESHAPE;
    if (N > 65535 || (int64_t)H * W > (1 << 28)) return XMC_ESHAPE;          // grid.y; pixel indices of one image in an int
    if ((reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(params) & 15)) return XMC_EALIGN;
    return 0;
}
}  // namespace

extern "C" int xmc_diffaug_sums(const void* x, const float* params, float* parts, int N, int H, int W, int C, int cut, int transposed,
                                int dtype, void* stream) {
    const int rc = check_args(x, params, N, H, W, C, cut, dtype);
    if (rc) return rc;
    if (!parts) return XMC_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(diffaug_parts(H * W), N), block(NT);
#define XMC_DA_SUMS(DT, TR) hipLaunchKernelGGL((diffaug_sums_kernel<DT, TR>), grid, block, 0, st, x, params, parts, H, W, C, cut)
    if (dtype == XMC_BF16) { if (transposed) XMC_DA_SUMS(XMC_BF16, true); else XMC_DA_SUMS(XMC_BF16, false); }
    else { if (transposed) XMC_DA_SUMS(XMC_F32, true); else XMC_DA_SUMS(XMC_F32, false); }
#undef XMC_DA_SUMS
    xmc_note_kernel("diffaug_sums_kernel<%s,%d>", dtype == XMC_BF16 ? "h16" : "f32", transposed ? 1 : 0);
    XMC_LAUNCH_CHECK();
    return 0;
}

extern "C" int xmc_diffaug_apply(const void* x, const float* params, const float* parts, void* y, int N, int H, int W, int C, int cut,
                                 int transposed, int linear_only, int dtype, void* stream) {
    const int rc = check_args(x, params, N, H, W, C, cut, dtype);
    if (rc) return rc;
    if (!y || y == x) return XMC_EINVAL;
    if (reinterpret_cast<uintptr_t>(y) & 15) return XMC_EALIGN;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int HW = H * W, nparts = diffaug_parts(HW);
    const dim3 grid(nparts, N), block(NT);                                     // (the same walk as the sums pass: PIX_PER_THREAD trips)
    const int lin = linear_only ? 1 : 0;
#define XMC_DA_APPLY(DT, TR) hipLaunchKernelGGL((diffaug_apply_kernel<DT, TR>), grid, block, 0, st, x, params, parts, y, H, W, C, cut, nparts, lin)
    if (dtype == XMC_BF16) { if (transposed) XMC_DA_APPLY(XMC_BF16, true); else XMC_DA_APPLY(XMC_BF16, false); }
    else { if (transposed) XMC_DA_APPLY(XMC_F32, true); else XMC_DA_APPLY(XMC_F32, false); }
#undef XMC_DA_APPLY
    xmc_note_kernel("diffaug_apply_kernel<%s,%d>", dtype == XMC_BF16 ? "h16" : "f32", transposed ? 1 : 0);
    XMC_LAUNCH_CHECK();
    return 0;
}
