// The two pointwise stages of the frozen VGG-19 (xmc_gan_amd/vgg.py) that no other kernel file has: ImageNet normalisation of the engine
// image and the fused ReLU + 2x2 max pool, each with its backward (include/xmc_gan_hip.h, "VGG-19 feature loss").
// Streaming kernels over NHWC tensors of up to 2 GB: one 8-channel unit (16 bytes in the 16-bit builds) per access, every output unit
// written by exactly one thread, no reduction across threads, so the same inputs give the same bytes.  Indices are 64-bit.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int UN = 4;                    // units per thread and step of the flat kernels, all requested before the first use
constexpr int GRID_CAP = 256 * 16;       // grid-stride beyond this many workgroups

inline int nblocks(int64_t items, int per_block) {
    int64_t b = (items + per_block - 1) / per_block;
    if (b < 1) b = 1;
    return (int)(b > GRID_CAP ? GRID_CAP : b);
}

// torchvision's ImageNet statistics.  The image arrives in [-1, 1]; VGG was trained on ((x + 1) / 2 - mean) / std.
// The shift CANNOT be folded into conv1_1's bias: conv1_1 pads with zeros in the NORMALISED domain, and a zero there is the raw value
// 2 mean - 1, not 0 -- a folded bias would be right in the interior and wrong in the one-pixel border of every image.  (The scale alone
// could go into the weights; the shift cannot, so the stage stays a pass of its own over the 8-channel image, 1/8 of conv1_1's output.)
struct PrepConst { float off[3], std[3], bwd[3]; };
inline PrepConst prep_const() {
    const double mean[3] = {0.485, 0.456, 0.406}, sd[3] = {0.229, 0.224, 0.225};
    PrepConst c;
    for (int k = 0; k < 3; ++k) {
        c.off[k] = (float)(0.5 - mean[k]);
        c.std[k] = (float)sd[k];
        c.bwd[k] = (float)(0.5 / sd[k]);
    }
    return c;
}

// y_c = (x_c / 2 + (1/2 - mean_c)) / std_c for c < 3, 0 for the five padding channels (BWD: dx_c = dy_c * (1/2) / std_c)
template <int DT, bool BWD>
__global__ void vgg_prep_kernel(const void* x, void* y, int64_t n8, PrepConst c) {
    for (int64_t base = (int64_t)blockIdx.x * (NT * UN); base < n8; base += (int64_t)gridDim.x * (NT * UN)) {
        float v[UN][8];
#pragma unroll
        for (int j = 0; j < UN; ++j) {
            const int64_t i = base + j * NT + threadIdx.x;
            if (i < n8) Vec8<DT>::load(x, i, v[j]);
        }
#pragma unroll
        for (int j = 0; j < UN; ++j) {
            const int64_t i = base + j * NT + threadIdx.x;
            if (i < n8) {
#pragma unroll
                for (int k = 0; k < 3; ++k) v[j][k] = BWD ? v[j][k] * c.bwd[k] : __builtin_fmaf(v[j][k], 0.5f, c.off[k]) / c.std[k];
#pragma unroll
                for (int k = 3; k < 8; ++k) v[j][k] = 0.f;
                Vec8<DT>::store(y, i, v[j]);
            }
        }
    }
}

// One thread per (output pixel, 8-channel unit): the four units of its window are requested together.  Scan order of the window is
// (0,0) (0,1) (1,0) (1,1), and "the maximum" is torch's: the first position whose value is greater than everything before it.
__device__ __forceinline__ int64_t window_unit(int64_t i, int OH, int OW, int C8, int64_t* row_units) {
    const int cc = (int)(i % C8);
    int64_t p = i / C8;
    const int ow = (int)(p % OW);
    p /= OW;
    const int oh = (int)(p % OH);
    const int64_t n = p / OH;
    *row_units = (int64_t)(2 * OW) * C8;
    return ((n * (2 * OH) + 2 * oh) * (int64_t)(2 * OW) + 2 * ow) * C8 + cc;
}

template <int DT>
__global__ void relu_maxpool2_fwd_kernel(const void* z, void* p, int64_t total, int OH, int OW, int C8) {
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
        int64_t row;
        const int64_t u = window_unit(i, OH, OW, C8, &row);
        float a[8], b[8], c[8], d[8], m[8];
        Vec8<DT>::load(z, u, a);
        Vec8<DT>::load(z, u + C8, b);
        Vec8<DT>::load(z, u + row, c);
        Vec8<DT>::load(z, u + row + C8, d);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float t = a[k];
            t = b[k] > t ? b[k] : t;
            t = c[k] > t ? c[k] : t;
            t = d[k] > t ? d[k] : t;
            m[k] = t > 0.f ? t : 0.f;
        }
        Vec8<DT>::store(p, i, m);
    }
}

// dz = dp at the first position (scan order) that holds the window's maximum when that maximum is > 0, and 0 at every other position:
// max_pool2d's tie rule composed with ReLU's zero gradient at <= 0.  The position is recomputed from z; no index tensor exists.
template <int DT>
__global__ void relu_maxpool2_bwd_kernel(const void* z, const void* dp, void* dz, int64_t total, int OH, int OW, int C8) {
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
        int64_t row;
        const int64_t u = window_unit(i, OH, OW, C8, &row);
        float a[8], b[8], c[8], d[8], g[8];
        Vec8<DT>::load(z, u, a);
        Vec8<DT>::load(z, u + C8, b);
        Vec8<DT>::load(z, u + row, c);
        Vec8<DT>::load(z, u + row + C8, d);
        Vec8<DT>::load(dp, i, g);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float t = a[k];
            int at = 0;
            if (b[k] > t) { t = b[k]; at = 1; }
            if (c[k] > t) { t = c[k]; at = 2; }
            if (d[k] > t) { t = d[k]; at = 3; }
            const float gk = t > 0.f ? g[k] : 0.f;
            a[k] = at == 0 ? gk : 0.f;
            b[k] = at == 1 ? gk : 0.f;
            c[k] = at == 2 ? gk : 0.f;
            d[k] = at == 3 ? gk : 0.f;
        }
        Vec8<DT>::store(dz, u, a);
        Vec8<DT>::store(dz, u + C8, b);
        Vec8<DT>::store(dz, u + row, c);
        Vec8<DT>::store(dz, u + row + C8, d);
    }
}

inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

// true when the product of the (positive) factors exceeds 2^40 units, without ever forming a product that leaves an int64
constexpr int64_t MAX_UNITS = (int64_t)1 << 40;
inline bool too_many_units(int a, int b, int c, int d = 1) {
    int64_t n = a;
    for (int f : {b, c, d}) {
        if (n > MAX_UNITS / f) return true;
        n *= f;
    }
    return false;
}

int check_prep(const void* x, const void* y, int N, int H, int W, int dtype) {
    if (!x || !y || (dtype != XMC_BF16 && dtype != XMC_F32)) return XMC_EINVAL;
    if (N < 1 || H < 1 || W < 1 || too_many_units(N, H, W)) return XMC_ESHAPE;
    if (misaligned(x) || misaligned(y)) return XMC_EALIGN;
    return 0;
}

int check_pool(const void* z, const void* p, int N, int H, int W, int C, int dtype) {
    if (!z || !p || (dtype != XMC_BF16 && dtype != XMC_F32)) return XMC_EINVAL;
    if (N < 1 || H < 2 || W < 2 || C < 8 || (C % 8) || (H % 2) || (W % 2) || too_many_units(N, H, W, C / 8)) return XMC_ESHAPE;
    if (misaligned(z) || misaligned(p)) return XMC_EALIGN;
    return 0;
}

template <bool BWD>
int launch_prep(const void* x, void* y, int N, int H, int W, int dtype, void* stream) {
    const int rc = check_prep(x, y, N, H, W, dtype);
    if (rc) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t n8 = (int64_t)N * H * W;
    const dim3 grid(nblocks(n8, NT * UN)), block(NT);
    const PrepConst c = prep_const();
    if (dtype == XMC_BF16) hipLaunchKernelGGL((vgg_prep_kernel<XMC_BF16, BWD>), grid, block, 0, st, x, y, n8, c);
    else hipLaunchKernelGGL((vgg_prep_kernel<XMC_F32, BWD>), grid, block, 0, st, x, y, n8, c);
    xmc_note_kernel("vgg_prep_kernel<%s,%d>", dtype == XMC_BF16 ? "h16" : "f32", BWD ? 1 : 0);
    XMC_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int xmc_vgg_prep_fwd(const void* x, void* y, int N, int H, int W, int dtype, void* stream) {
    return launch_prep<false>(x, y, N, H, W, dtype, stream);
}

extern "C" int xmc_vgg_prep_bwd(const void* dy, void* dx, int N, int H, int W, int dtype, void* stream) {
    return launch_prep<true>(dy, dx, N, H, W, dtype, stream);
}

extern "C" int xmc_relu_maxpool2_fwd(const void* z, void* p, int N, int H, int W, int C, int dtype, void* stream) {
    const int rc = check_pool(z, p, N, H, W, C, dtype);
    if (rc) return rc;
    if (p == z) return XMC_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int OH = H / 2, OW = W / 2, C8 = C / 8;
    const int64_t total = (int64_t)N * OH * OW * C8;
    const dim3 grid(nblocks(total, NT)), block(NT);
    if (dtype == XMC_BF16) hipLaunchKernelGGL((relu_maxpool2_fwd_kernel<XMC_BF16>), grid, block, 0, st, z, p, total, OH, OW, C8);
    else hipLaunchKernelGGL((relu_maxpool2_fwd_kernel<XMC_F32>), grid, block, 0, st, z, p, total, OH, OW, C8);
    xmc_note_kernel("relu_maxpool2_fwd_kernel<%s>", dtype == XMC_BF16 ? "h16" : "f32");
    XMC_LAUNCH_CHECK();
    return 0;
}

extern "C" int xmc_relu_maxpool2_bwd(const void* z, const void* dp, void* dz, int N, int H, int W, int C, int dtype, void* stream) {
    const int rc = check_pool(z, dp, N, H, W, C, dtype);
    if (rc) return rc;
    if (!dz || dz == z || dz == dp) return XMC_EINVAL;
    if (misaligned(dz)) return XMC_EALIGN;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int OH = H / 2, OW = W / 2, C8 = C / 8;
    const int64_t total = (int64_t)N * OH * OW * C8;
    const dim3 grid(nblocks(total, NT)), block(NT);
    if (dtype == XMC_BF16) hipLaunchKernelGGL((relu_maxpool2_bwd_kernel<XMC_BF16>), grid, block, 0, st, z, dp, dz, total, OH, OW, C8);
    else hipLaunchKernelGGL((relu_maxpool2_bwd_kernel<XMC_F32>), grid, block, 0, st, z, dp, dz, total, OH, OW, C8);
    xmc_note_kernel("relu_maxpool2_bwd_kernel<%s>", dtype == XMC_BF16 ? "h16" : "f32");
    XMC_LAUNCH_CHECK();
    return 0;
}
