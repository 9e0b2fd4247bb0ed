// The parts of the FID evaluation (xmc_gan_amd/fid.py) that are not convolutions -- the reference leaves all of this to pytorch_fid
// (train_gan.py:389, calculate_fid_given_paths); nothing here is on the training step.  Everything is f32 or wider.
//
//   resize_u8   uint8 [N,H,W,3] (what xmc_image_to_u8 writes and PIL reads) -> f32 engine image [N,OH,OW,8]: bilinear with PyTorch's
//               align_corners=False rule (src = max((dst + 0.5) * in / out - 0.5, 0), upper neighbour clamped to the edge, no antialias),
//               then 2 * (v / 255) - 1; channels 3..7 are zero.  The source coordinate is worked out in f64 (one per row and column of a
//               thread's pixel), the blend in f32 on the byte values: with OH == H and OW == W both weights are exactly 1 and 0 and the
//               result EQUALS 2 * (b / 255) - 1.
//   resize_f32  f32 NCHW [N,3,H,W] (what a generator returns) -> the same engine image by the same coordinate rule, values not rescaled: the
//               front end of the DAMSM image encoder (xmc_gan/model/encoder.py CNN_ENCODER).  Equal sizes: weights 1 and 0, the input exactly.
//   pool3x3     3x3 max pool / average over the in-image pixels of the window (count_include_pad=False) on f32 [N,H,W,C], C % 4 == 0:
//               stride 1 with padding 1 (OH = H) or stride 2 without padding (OH = (H - 3) / 2 + 1, floor).  One thread per output pixel and
//               16-byte channel unit.  Mode 2 (stride 1 only) divides the same sum by 9 (count_include_pad=True: torchvision's branch_pool).
//   moments     running f64 statistics of a batch of f32 feature rows X [B,D]: sum[d] += sum_b X[b][d], outer[i][j] += sum_b X[b][i] X[b][j],
//               products and sums in f64.  Every output element has ONE owner thread that adds its batch rows in order: no atomics, the same
//               bytes for the same batches every time.  64 x 64 tiles of `outer`, 4 x 4 elements per thread, the two 64-column strips of X
//               staged through LDS 16 rows at a time.
#include "common.h"

namespace {
constexpr int NT = 256;

struct Lerp { int i0, i1; float l; };
__device__ __forceinline__ Lerp src_coord(int o, int in, int out) {
    double s = ((double)o + 0.5) * ((double)in / (double)out) - 0.5;
    if (s < 0.0) s = 0.0;
    Lerp r;
    r.i0 = (int)s;
    if (r.i0 > in - 1) r.i0 = in - 1;
    r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
    r.l = (float)(s - (double)r.i0);
    return r;
}

__global__ void __launch_bounds__(NT) fid_resize_u8_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int N, int H, int W, int OH,
                                                          int OW) {
    const int64_t P = (int64_t)N * OH * OW;
    for (int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x; p < P; p += (int64_t)gridDim.x * NT) {
        const int ox = (int)(p % OW);
        const int64_t q = p / OW;
        const int oy = (int)(q % OH), n = (int)(q / OH);
        const Lerp ly = src_coord(oy, H, OH), lx = src_coord(ox, W, OW);
        const uint8_t* img = src + (size_t)n * H * W * 3;
        const uint8_t* p00 = img + ((size_t)ly.i0 * W + lx.i0) * 3;
        const uint8_t* p01 = img + ((size_t)ly.i0 * W + lx.i1) * 3;
        const uint8_t* p10 = img + ((size_t)ly.i1 * W + lx.i0) * 3;
        const uint8_t* p11 = img + ((size_t)ly.i1 * W + lx.i1) * 3;
        const float wx1 = lx.l, wx0 = 1.f - lx.l, wy1 = ly.l, wy0 = 1.f - ly.l;
        f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float top = wx0 * (float)p00[c] + wx1 * (float)p01[c];
            const float bot = wx0 * (float)p10[c] + wx1 * (float)p11[c];
            const float v = wy0 * top + wy1 * bot;
            lo[c] = 2.f * (v / 255.f) - 1.f;
        }
        f32x4* o = reinterpret_cast<f32x4*>(dst) + (size_t)p * 2;
        o[0] = lo; o[1] = hi;
    }
}

__global__ void __launch_bounds__(NT) resize_bilinear_f32_kernel(const float* __restrict__ src, float* __restrict__ dst, int N, int H, int W, int OH,
                                                                int OW) {
    const int64_t P = (int64_t)N * OH * OW;
    const size_t plane = (size_t)H * W;
    for (int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x; p < P; p += (int64_t)gridDim.x * NT) {
        const int ox = (int)(p % OW);
        const int64_t q = p / OW;
        const int oy = (int)(q % OH), n = (int)(q / OH);
        const Lerp ly = src_coord(oy, H, OH), lx = src_coord(ox, W, OW);
        const float* img = src + (size_t)n * 3 * plane;
        const size_t o00 = (size_t)ly.i0 * W + lx.i0, o01 = (size_t)ly.i0 * W + lx.i1, o10 = (size_t)ly.i1 * W + lx.i0, o11 = (size_t)ly.i1 * W + lx.i1;
        const float wx1 = lx.l, wx0 = 1.f - lx.l, wy1 = ly.l, wy0 = 1.f - ly.l;
        f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* pl = img + (size_t)c * plane;
            const float top = wx0 * pl[o00] + wx1 * pl[o01];
            const float bot = wx0 * pl[o10] + wx1 * pl[o11];
            lo[c] = wy0 * top + wy1 * bot;
        }
        f32x4* o = reinterpret_cast<f32x4*>(dst) + (size_t)p * 2;
        o[0] = lo; o[1] = hi;
    }
}

// MODE 0: max, 1: sum / number of in-image pixels, 2: sum / 9.  STRIDE 1 (padding 1) or 2 (no padding).
template <int MODE, int STRIDE>
__global__ void __launch_bounds__(NT) pool3x3_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int H, int W, int C4, int OH, int OW) {
    const int64_t items = (int64_t)N * OH * OW * C4;
    const f32x4* __restrict__ x4 = reinterpret_cast<const f32x4*>(x);
    f32x4* __restrict__ y4 = reinterpret_cast<f32x4*>(y);
    for (int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x; t < items; t += (int64_t)gridDim.x * NT) {
        const int c = (int)(t % C4);
        int64_t q = t / C4;
        const int ow = (int)(q % OW);
        q /= OW;
        const int oh = (int)(q % OH), n = (int)(q / OH);
        const int h0 = STRIDE == 1 ? oh - 1 : 2 * oh, w0 = STRIDE == 1 ? ow - 1 : 2 * ow;
        f32x4 acc = MODE == 0 ? f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY} : f32x4{0.f, 0.f, 0.f, 0.f};
        int cnt = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int h = h0 + i;
            if ((unsigned)h >= (unsigned)H) continue;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int w = w0 + j;
                if ((unsigned)w >= (unsigned)W) continue;
                const f32x4 v = x4[(((size_t)n * H + h) * W + w) * C4 + c];
                if (MODE == 0) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[k] = fmaxf(acc[k], v[k]);
                } else {
                    acc += v;
                }
                ++cnt;
            }
        }
        if (MODE == 1) {
            const float inv = (float)cnt;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = acc[k] / inv;
        }
        if (MODE == 2) {
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = acc[k] / 9.f;
        }
        y4[t] = acc;
    }
}

constexpr int MT = 64, MKB = 16;          // tile of `outer`, batch rows per LDS stage
__global__ void __launch_bounds__(NT) fid_outer_kernel(const float* __restrict__ x, double* __restrict__ outer, int B, int D) {
    __shared__ float si[MKB][MT], sj[MKB][MT];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int i0 = blockIdx.y * MT, j0 = blockIdx.x * MT;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    for (int b0 = 0; b0 < B; b0 += MKB) {
#pragma unroll
        for (int r = 0; r < MKB * MT / NT; ++r) {
            const int e = tid + r * NT, row = e / MT, col = e % MT;
            const int b = b0 + row;
            si[row][col] = (b < B && i0 + col < D) ? x[(size_t)b * D + i0 + col] : 0.f;
            sj[row][col] = (b < B && j0 + col < D) ? x[(size_t)b * D + j0 + col] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < MKB; ++k) {
            double vi[4], vj[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) { vi[a] = (double)si[k][ty * 4 + a]; vj[a] = (double)sj[k][tx * 4 + a]; }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = fma(vi[a], vj[b], acc[a][b]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int i = i0 + ty * 4 + a;
        if (i >= D) continue;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int j = j0 + tx * 4 + b;
            if (j < D) outer[(size_t)i * D + j] += acc[a][b];
        }
    }
}

__global__ void __launch_bounds__(NT) fid_sum_kernel(const float* __restrict__ x, double* __restrict__ sum, int B, int D) {
    const int d = blockIdx.x * NT + threadIdx.x;
    if (d >= D) return;
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += (double)x[(size_t)b * D + d];
    sum[d] += s;
}

inline int blocks_for(int64_t items, int cap) {
    const int64_t b = (items + NT - 1) / NT;
    return b < 1 ? 1 : (b < cap ? (int)b : cap);
}
}  // namespace

extern "C" int xmc_fid_resize_u8(const uint8_t* src, float* dst, int N, int H, int W, int OH, int OW, void* stream) {
    if (!src || !dst) return XMC_EINVAL;
    if (N < 1 || H < 1 || W < 1 || OH < 1 || OW < 1) return XMC_ESHAPE;
    if ((int64_t)H * W > (int64_t)1 << 30 || (int64_t)OH * OW > (int64_t)1 << 30) return XMC_ESHAPE;
    if (reinterpret_cast<uintptr_t>(dst) & 15) return XMC_EALIGN;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(fid_resize_u8_kernel, dim3(blocks_for((int64_t)N * OH * OW, 16384)), dim3(NT), 0, st, src, dst, N, H, W, OH, OW);
    xmc_note_kernel("fid_resize_u8_kernel");
    XMC_LAUNCH_CHECK();
    return 0;
}

extern "C" int xmc_resize_bilinear_f32(const float* src, float* dst, int N, int H, int W, int OH, int OW, void* stream) {
    if (!src || !dst) return XMC_EINVAL;
    if (N < 1 || H < 1 || W < 1 || OH < 1 || OW < 1) return XMC_ESHAPE;
    if ((int64_t)H * W > (int64_t)1 << 30 || (int64_t)OH * OW > (int64_t)1 << 30) return XMC_ESHAPE;
    if ((reinterpret_cast<uintptr_t>(dst) & 15) || (reinterpret_cast<uintptr_t>(src) & 3)) return XMC_EALIGN;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(resize_bilinear_f32_kernel, dim3(blocks_for((int64_t)N * OH * OW, 16384)), dim3(NT), 0, st, src, dst, N, H, W, OH, OW);
    xmc_note_kernel("resize_bilinear_f32_kernel");
    XMC_LAUNCH_CHECK();
    return 0;
}

extern "C" int xmc_pool3x3(const float* x, float* y, int N, int H, int W, int C, int mode, int stride, void* stream) {
    if (!x || !y || (mode != XMC_POOL_MAX && mode != XMC_POOL_AVG_VALID && mode != XMC_POOL_AVG_PAD) || (stride != 1 && stride != 2)) return XMC_EINVAL;
    if (mode == XMC_POOL_AVG_PAD && stride != 1) return XMC_EINVAL;
    if (N < 1 || H < 1 || W < 1 || C < 4) return XMC_ESHAPE;
    if (stride == 2 && (H < 3 || W < 3)) return XMC_ESHAPE;               // no whole window: the output would be empty
    if (C % 4 != 0 || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15)) return XMC_EALIGN;
    const int OH = stride == 1 ? H : (H - 3) / 2 + 1, OW = stride == 1 ? W : (W - 3) / 2 + 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(blocks_for((int64_t)N * OH * OW * (C / 4), 1 << 20)), block(NT);
#define XMC_POOL_GO(M_, S_) hipLaunchKernelGGL((pool3x3_kernel<M_, S_>), grid, block, 0, st, x, y, N, H, W, C / 4, OH, OW)
    if (mode == XMC_POOL_MAX) { if (stride == 1) XMC_POOL_GO(0, 1); else XMC_POOL_GO(0, 2); }
    else if (mode == XMC_POOL_AVG_VALID) { if (stride == 1) XMC_POOL_GO(1, 1); else XMC_POOL_GO(1, 2); }
    else XMC_POOL_GO(2, 1);
#undef XMC_POOL_GO
    xmc_note_kernel("pool3x3_kernel<%d, %d>", mode, stride);
    XMC_LAUNCH_CHECK();
    return 0;
}

extern "C" int xmc_fid_moments(const float* x, double* sum, double* outer, int B, int D, void* stream) {
    if (!x || !sum || !outer) return XMC_EINVAL;
    if (B < 1 || D < 1 || D > 32768) return XMC_ESHAPE;
    if ((reinterpret_cast<uintptr_t>(x) & 3) || ((reinterpret_cast<uintptr_t>(sum) | reinterpret_cast<uintptr_t>(outer)) & 7)) return XMC_EALIGN;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int T = (D + MT - 1) / MT;
    hipLaunchKernelGGL(fid_sum_kernel, dim3((D + NT - 1) / NT), dim3(NT), 0, st, x, sum, B, D);
    XMC_LAUNCH_CHECK();
    hipLaunchKernelGGL(fid_outer_kernel, dim3(T, T), dim3(NT), 0, st, x, outer, B, D);
    xmc_note_kernel("fid_outer_kernel");
    XMC_LAUNCH_CHECK();
    return 0;
}
