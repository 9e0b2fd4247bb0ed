// The image tail of sampling (not in the reference as device code): the engine's [N,H,W,8] image -> the uint8 pixels that the host code
// used to make from an f32 NCHW copy.  Channels 0..2 are read, 3..7 ignored; a 16-bit pixel is read as its first 8 bytes, an f32 pixel as
// its first 16 of 32.
//
//   to_u8     trunc((x + 1) * 127.5), clamped to [0, 255], NaN -> 0: utils/visual.to_uint8_hwc, what eval() writes per image
//             (reference train_gan.py:366-379).  y [N,H,W,3].
//   minmax    per-image partial (min, max) over channels 0..2, one pair per workgroup, no atomics (the scheme of augment.hip's sums pass):
//             XMC_DIFFAUG_PARTS slots per image, of which the first image_parts(H*W) are written.
//   grid_u8   the bytes utils/visual.save_image(x, normalize=True, scale_each=True) encodes: every image min-max scaled on its own,
//             g = clamp((x - lo) / max(hi - lo, 1e-5), 0, 1), u8 = trunc(clamp(g * 255 + 0.5, 0, 255)), laid out as make_grid does, padding
//             and empty cells 0.  Each pass reads its image once.
//
// The arithmetic is f32 with every operation rounded on its own (no contraction of g * 255 + 0.5 into an fma; `/` is the correctly
// rounded division, hipcc's default for f32), which is what makes the result EQUAL to the numpy code it replaces rather than close to it.
//
// Output alignment: 3-byte pixels put most row starts off a 4-byte boundary, and a caller may hand in any byte address.  None is refused:
// a run of pixels whose first byte is at address a is written as (a & 3) single pixels -- after k pixels the address is a + 3k, a multiple
// of 4 for k = a & 3 -- then groups of four pixels as three aligned 32-bit words, then at most three single pixels.  Nothing is written
// outside the 3 * pixels bytes of the run.
#include "common.h"

namespace {
constexpr int NT = 256;
constexpr int PIX_PER_THREAD = 4;

inline int image_parts(int64_t HW) {
    const int64_t p = (HW + NT * PIX_PER_THREAD - 1) / (NT * PIX_PER_THREAD);
    return p < XMC_DIFFAUG_PARTS ? (int)p : XMC_DIFFAUG_PARTS;
}

// channels 0..2 of pixel `pix` as floats
template <int DT> __device__ __forceinline__ void load_rgb(const void* p, size_t pix, float (&v)[3]);
template <> __device__ __forceinline__ void load_rgb<XMC_BF16>(const void* p, size_t pix, float (&v)[3]) {
    const bf16x4 t = reinterpret_cast<const bf16x4*>(p)[pix * 2];
    v[0] = (float)t[0]; v[1] = (float)t[1]; v[2] = (float)t[2];
}
template <> __device__ __forceinline__ void load_rgb<XMC_F32>(const void* p, size_t pix, float (&v)[3]) {
    const f32x4 t = reinterpret_cast<const f32x4*>(p)[pix * 2];
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2];
}

// fmaxf(NaN, 0) == 0: NaN -> 0; the conversion truncates
__device__ __forceinline__ uint8_t sat_u8(float v) { return (uint8_t)(int)fminf(fmaxf(v, 0.f), 255.f); }
// (contraction is switched off where a product feeds a sum: the library is built with it on, and __fmul_rn / __fadd_rn are plain `*` / `+`
// to this compiler, so they would not keep g * 255 + 0.5 from becoming one fma)
__device__ __forceinline__ uint8_t unit_u8(float x) {
#pragma clang fp contract(off)
    const float s = x + 1.0f;
    return sat_u8(s * 127.5f);
}
__device__ __forceinline__ uint8_t scaled_u8(float x, float lo, float d) {
#pragma clang fp contract(off)
    const float q = (x - lo) / d;
    const float g = fminf(fmaxf(q, 0.f), 1.f);
    const float m = g * 255.0f;
    return sat_u8(m + 0.5f);
}

struct __attribute__((aligned(4))) Word3 { uint32_t a, b, c; };
// 12 bytes (four pixels) at a 4-byte aligned address
__device__ __forceinline__ void store_px4(uint8_t* dst, const uint8_t (&b)[12]) {
    Word3 w;
    w.a = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
    w.b = (uint32_t)b[4] | ((uint32_t)b[5] << 8) | ((uint32_t)b[6] << 16) | ((uint32_t)b[7] << 24);
    w.c = (uint32_t)b[8] | ((uint32_t)b[9] << 8) | ((uint32_t)b[10] << 16) | ((uint32_t)b[11] << 24);
    *reinterpret_cast<Word3*>(dst) = w;
}

// A run of `n` pixels as work items: `head` single pixels, `quads` groups of four, `tail` single pixels (see the note on alignment above).
struct Run { int64_t head, quads, tail; };
__device__ __forceinline__ Run split_run(const uint8_t* first, int64_t n) {
    Run r;
    const int64_t mis = (int64_t)(reinterpret_cast<uintptr_t>(first) & 3);
    r.head = mis < n ? mis : n;
    r.quads = (n - r.head) >> 2;
    r.tail = n - r.head - 4 * r.quads;
    return r;
}

// 1-D grid, grid-stride over the work items of the one run of P = N*H*W pixels
template <int DT>
__global__ void __launch_bounds__(NT) image_to_u8_kernel(const void* __restrict__ x, uint8_t* __restrict__ y, int64_t P) {
    const Run r = split_run(y, P);
    const int64_t items = r.head + r.quads + r.tail;
    for (int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x; t < items; t += (int64_t)gridDim.x * NT) {
        if (t >= r.head && t < r.head + r.quads) {
            const int64_t p0 = r.head + 4 * (t - r.head);
            uint8_t b[12];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float v[3];
                load_rgb<DT>(x, (size_t)(p0 + q), v);
#pragma unroll
                for (int k = 0; k < 3; ++k) b[3 * q + k] = unit_u8(v[k]);
            }
            store_px4(y + 3 * p0, b);
        } else {
            const int64_t p = t < r.head ? t : r.head + 4 * r.quads + (t - r.head - r.quads);
            float v[3];
            load_rgb<DT>(x, (size_t)p, v);
#pragma unroll
            for (int k = 0; k < 3; ++k) y[3 * p + k] = unit_u8(v[k]);
        }
    }
}

// grid (N, parts): workgroup (n, part) takes every parts-th stretch of NT pixels of image n and writes parts[n][part] = (min, max)
template <int DT>
__global__ void __launch_bounds__(NT) image_minmax_kernel(const void* __restrict__ x, float* __restrict__ parts, int HW) {
    __shared__ float red[2][NT / 64];
    const int n = blockIdx.x;
    float lo = INFINITY, hi = -INFINITY;
    for (int pix = blockIdx.y * NT + threadIdx.x; pix < HW; pix += gridDim.y * NT) {
        float v[3];
        load_rgb<DT>(x, (size_t)n * HW + pix, v);
        lo = fminf(lo, fminf(v[0], fminf(v[1], v[2])));
        hi = fmaxf(hi, fmaxf(v[0], fmaxf(v[1], v[2])));
    }
    lo = -wave_max(-lo);
    hi = wave_max(hi);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = lo; red[1][threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) { lo = fminf(lo, red[0][w]); hi = fmaxf(hi, red[1][w]); }
        float* o = parts + ((size_t)n * XMC_DIFFAUG_PARTS + blockIdx.y) * 2;
        o[0] = lo; o[1] = hi;
    }
}

// The grid is tiled by one region per cell: cell (yy, xx) owns the (H + pad) x (W + pad) pixels from its top-left padding corner on, the
// last row / column of cells the closing padding as well.  Workgroup (cell, part) writes every part-th stretch of its region's work items;
// a region row of rw pixels is one run (3 + ceil(rw / 4) + 3 item slots, the unused ones skipped).  Cells past the last image write zeros.
struct GridGeom { int H, W, pad, xmaps, ymaps, Wg, nparts; };
template <int DT>
__global__ void __launch_bounds__(NT) image_grid_u8_kernel(const void* __restrict__ x, const float* __restrict__ parts, uint8_t* __restrict__ grid,
                                                           int N, GridGeom G) {
    __shared__ float range[2];
    const int cell = blockIdx.x, yy = cell / G.xmaps, xx = cell - yy * G.xmaps;
    const bool live = cell < N;
    if (live) {                      // the image's partials, combined by the first wave (min and max do not depend on the order)
        if (threadIdx.x < 64) {
            const bool has = (int)threadIdx.x < G.nparts;
            const float* p = parts + ((size_t)cell * XMC_DIFFAUG_PARTS + threadIdx.x) * 2;
            const float lo = -wave_max(has ? -p[0] : -INFINITY), hi = wave_max(has ? p[1] : -INFINITY);
            if (threadIdx.x == 0) { range[0] = lo; range[1] = hi; }
        }
        __syncthreads();
    }
    const float lo = live ? range[0] : 0.f;
    const float d = live ? fmaxf(range[1] - lo, 1e-5f) : 1.f;
    const int h = G.H + G.pad, w = G.W + G.pad;
    const int rh = h + (yy == G.ymaps - 1 ? G.pad : 0), rw = w + (xx == G.xmaps - 1 ? G.pad : 0);
    const int slots = 6 + ((rw + 3) >> 2);
    const int64_t total = (int64_t)rh * slots;
    const size_t HW = (size_t)G.H * G.W;

    auto pixel = [&](int i, int c, uint8_t* out) {       // region pixel (row i - pad of the image, column c - pad) -> 3 bytes
        const int ii = i - G.pad, jj = c - G.pad;
        if (live && ii >= 0 && ii < G.H && jj >= 0 && jj < G.W) {
            float v[3];
            load_rgb<DT>(x, (size_t)cell * HW + (size_t)ii * G.W + jj, v);
#pragma unroll
            for (int k = 0; k < 3; ++k) out[k] = scaled_u8(v[k], lo, d);
        } else {
            out[0] = out[1] = out[2] = 0;
        }
    };

    for (int64_t f = (int64_t)blockIdx.y * NT + threadIdx.x; f < total; f += (int64_t)gridDim.y * NT) {
        const int i = (int)(f / slots), t = (int)(f - (int64_t)i * slots);
        uint8_t* row = grid + 3 * ((size_t)(yy * h + i) * G.Wg + (size_t)xx * w);
        const Run r = split_run(row, rw);
        const int nq = (rw + 3) >> 2;                    // quad slots: 3 .. 3 + nq
        if (t >= 3 && t < 3 + nq) {
            const int q = t - 3;
            if (q >= r.quads) continue;
            const int c0 = (int)r.head + 4 * q;
            uint8_t b[12];
#pragma unroll
            for (int k = 0; k < 4; ++k) pixel(i, c0 + k, b + 3 * k);
            store_px4(row + 3 * c0, b);
        } else {
            int c;
            if (t < 3) {
                if (t >= r.head) continue;
                c = t;
            } else {
                const int u = t - 3 - nq;
                if (u >= r.tail) continue;
                c = (int)(r.head + 4 * r.quads) + u;
            }
            uint8_t b[3];
            pixel(i, c, b);
            row[3 * c] = b[0]; row[3 * c + 1] = b[1]; row[3 * c + 2] = b[2];
        }
    }
}

// the header's order: pointers and dtype, then shapes, then alignment (nrow / padding: the grid's two extra shape arguments)
int check_image(const void* x, const void* out, int N, int H, int W, int dtype, int nrow = 1, int padding = 0) {
    if (!x || !out || (dtype != XMC_BF16 && dtype != XMC_F32)) return XMC_EINVAL;
    if (N < 1 || H < 1 || W < 1 || nrow < 1 || padding < 0) return XMC_ESHAPE;
    if ((int64_t)H * W > (int64_t)1 << 30) return XMC_ESHAPE;                 // pixel indices of one image in an int
    if (reinterpret_cast<uintptr_t>(x) & 15) return XMC_EALIGN;
    return 0;
}
inline int blocks_for(int64_t items, int per_block, int cap) {
    const int64_t b = (items + per_block - 1) / per_block;
    return b < 1 ? 1 : (b < cap ? (int)b : cap);
}
}  // namespace

extern "C" int xmc_image_to_u8(const void* x, uint8_t* y, int N, int H, int W, int dtype, void* stream) {
    const int rc = check_image(x, y, N, H, W, dtype);
    if (rc) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t P = (int64_t)N * H * W;
    const dim3 grid(blocks_for(P / 4 + 6, NT, 16384)), block(NT);
    if (dtype == XMC_BF16) hipLaunchKernelGGL((image_to_u8_kernel<XMC_BF16>), grid, block, 0, st, x, y, P);
    else hipLaunchKernelGGL((image_to_u8_kernel<XMC_F32>), grid, block, 0, st, x, y, P);
    xmc_note_kernel("image_to_u8_kernel<%s>", dtype == XMC_BF16 ? "h16" : "f32");
    XMC_LAUNCH_CHECK();
    return 0;
}

extern "C" int xmc_image_minmax(const void* x, float* parts, int N, int H, int W, int dtype, void* stream) {
    const int rc = check_image(x, parts, N, H, W, dtype);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(parts) & 3) return XMC_EALIGN;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(N, image_parts((int64_t)H * W)), block(NT);
    if (dtype == XMC_BF16) hipLaunchKernelGGL((image_minmax_kernel<XMC_BF16>), grid, block, 0, st, x, parts, H * W);
    else hipLaunchKernelGGL((image_minmax_kernel<XMC_F32>), grid, block, 0, st, x, parts, H * W);
    xmc_note_kernel("image_minmax_kernel<%s>", dtype == XMC_BF16 ? "h16" : "f32");
    XMC_LAUNCH_CHECK();
    return 0;
}

extern "C" int xmc_image_grid_u8(const void* x, const float* parts, uint8_t* grid_out, int N, int H, int W, int nrow, int padding, int dtype,
                                 void* stream) {
    if (!parts) return XMC_EINVAL;
    const int rc = check_image(x, grid_out, N, H, W, dtype, nrow, padding);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(parts) & 3) return XMC_EALIGN;
    GridGeom G;
    G.H = H; G.W = W;
    G.pad = N == 1 ? 0 : padding;                                              // make_grid hands a single image back as it is
    G.xmaps = nrow < N ? nrow : N;
    G.ymaps = (N + G.xmaps - 1) / G.xmaps;
    const int64_t Hg = (int64_t)(H + G.pad) * G.ymaps + G.pad, Wg = (int64_t)(W + G.pad) * G.xmaps + G.pad;
    if (Hg > INT32_MAX || Wg > INT32_MAX || (int64_t)G.xmaps * G.ymaps > INT32_MAX) return XMC_ESHAPE;
    G.Wg = (int)Wg;
    G.nparts = image_parts((int64_t)H * W);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t items = (int64_t)(H + 2 * G.pad) * (6 + ((W + 2 * G.pad + 3) >> 2));
    const dim3 grid(G.xmaps * G.ymaps, blocks_for(items, 2 * NT, XMC_DIFFAUG_PARTS)), block(NT);
    if (dtype == XMC_BF16) hipLaunchKernelGGL((image_grid_u8_kernel<XMC_BF16>), grid, block, 0, st, x, parts, grid_out, N, G);
    else hipLaunchKernelGGL((image_grid_u8_kernel<XMC_F32>), grid, block, 0, st, x, parts, grid_out, N, G);
    xmc_note_kernel("image_grid_u8_kernel<%s>", dtype == XMC_BF16 ? "h16" : "f32");
    XMC_LAUNCH_CHECK();
    return 0;
}
