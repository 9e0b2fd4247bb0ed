// The input side of a training step from a device-resident image pool (not in the reference as device code): RandomCrop +
// RandomHorizontalFlip + ToTensor + Normalize of xmc_gan/dataset.py as ONE gather over uint8 RGB images that already live in HBM.
//
//   out[b][c][y][x] = table[ pool[ offsets[i] + ((top + y) * w + left + (flip ? S-1-x : x)) * 3 + c ] ],   (i, top, left, flip) = params[b]
//
// `table` holds the host's to_normalized_tensor of the bytes 0..255, so the result EQUALS the host path whatever its division rounds to:
// the kernel does no arithmetic on a pixel's value, only a look-up.
//
// Access pattern.  A source row of a crop is 3*S bytes at an arbitrary byte address (3*w and 3*left are not multiples of 4).  A workgroup
// takes ROWS output rows of one crop: it copies the aligned 16-byte units that cover each row's segment into LDS (one `global_load_dwordx4`
// per unit, unit index clamped to the pool), then every thread takes four consecutive output pixels: the 12 source bytes come out of LDS as
// four aligned dwords funnel-shifted by the segment's misalignment, and go out as one float4 per colour plane -- consecutive lanes write
// consecutive 16-byte pieces of a plane's row.  No atomics, nothing written but `out`.
//
// Bounds.  The caller (ops.crop_flip_normalize) validates params on the host before it launches.  Independently of that, the kernel clamps the
// image index to [0, N) and every unit it loads to [0, pool_bytes / 16), so no params row can make it read outside offsets / hw / pool; its
// writes depend on (b, y, x) alone.
#include "common.h"

namespace {
constexpr int NT = 256;
constexpr int ROWS = 8;            // output rows per workgroup (S % 8 == 0: no partial group)
constexpr int S_MAX = 1024;           // 25.7 KB of LDS per workgroup at most

// units of 16 bytes that cover 3*S bytes starting at any misalignment 0..15
__host__ __device__ inline int row_units(int S) { return (3 * S + 15) / 16 + 1; }

// bytes [sh, sh + 4) of the little-endian pair (lo, hi), sh in 0..3
__device__ __forceinline__ uint32_t funnel(uint32_t lo, uint32_t hi, int sh) {
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * sh));
}

__global__ void __launch_bounds__(NT) crop_flip_normalize_kernel(const uint4* __restrict__ pool, int64_t pool_units,
                                                                 const int64_t* __restrict__ offsets, const int32_t* __restrict__ hw, int N,
                                                                 const int32_t* __restrict__ params, const float* __restrict__ table,
                                                                 float* __restrict__ out, int S) {
    extern __shared__ uint4 lds_units[];              // [ROWS][U] units, one spare unit, then the 256-entry table
    const int U = row_units(S);
    float* lut = reinterpret_cast<float*>(lds_units + ROWS * U + 1);
    const int groups = S / ROWS;
    const int b = blockIdx.x / groups, y0 = (blockIdx.x - b * groups) * ROWS;

    const int32_t* pr = params + (size_t)b * 4;
    int idx = pr[0];
    idx = idx < 0 ? 0 : (idx >= N ? N - 1 : idx);
    const int64_t top = pr[1], left = pr[2];
    const bool flip = pr[3] != 0;
    const int64_t w = hw[(size_t)idx * 2 + 1];
    const int64_t first = offsets[idx] + ((top + y0) * w + left) * 3;     // byte address of the first source byte of row y0

    lut[threadIdx.x] = table[threadIdx.x];                                // NT == 256 entries
    for (int t = threadIdx.x; t < ROWS * U; t += NT) {
        const int r = t / U, j = t - r * U;
        const int64_t a = first + (int64_t)r * w * 3;
        int64_t u = (a >> 4) + j;                                          // (arithmetic shift: floor for a negative address too)
        u = u < 0 ? 0 : (u >= pool_units ? pool_units - 1 : u);
        lds_units[t] = pool[u];
    }
    __syncthreads();

    const uint32_t* words = reinterpret_cast<const uint32_t*>(lds_units);
    const int quads = S / 4;
    for (int t = threadIdx.x; t < ROWS * quads; t += NT) {
        const int r = t / quads, q = t - r * quads;
        const int64_t a = first + (int64_t)r * w * 3;
        const int m = (int)(a & 15);                                       // the row's misalignment inside its first unit
        const int qs = flip ? quads - 1 - q : q;                           // source quad: pixels 4*qs .. 4*qs + 3 of the crop's row
        const int o = m + 12 * qs;                                         // byte offset of its 12 bytes inside the row's LDS image
        const uint32_t* p = words + r * (U * 4) + (o >> 2);
        const int sh = o & 3;
        const uint32_t d0 = p[0], d1 = p[1], d2 = p[2], d3 = p[3];         // (p[3] may be the next row's first word or the spare unit: shifted out)
        const uint32_t v[3] = {funnel(d0, d1, sh), funnel(d1, d2, sh), funnel(d2, d3, sh)};
        float px[4][3];
#pragma unroll
        for (int k = 0; k < 12; ++k) px[k / 3][k % 3] = lut[(v[k >> 2] >> (8 * (k & 3))) & 0xffu];
        const size_t row = (size_t)b * 3 * S + (size_t)(y0 + r);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float4 f;
            if (flip) f = make_float4(px[3][c], px[2][c], px[1][c], px[0][c]);
            else f = make_float4(px[0][c], px[1][c], px[2][c], px[3][c]);
            reinterpret_cast<float4*>(out + (row + (size_t)c * S) * S)[q] = f;
        }
    }
}
}  // namespace

extern "C" int xmc_crop_flip_normalize(const uint8_t* pool, int64_t pool_bytes, const int64_t* offsets, const int32_t* hw, int N,
                                       const int32_t* params, const float* table, float* out, int B, int S, void* stream) {
    if (!pool || !offsets || !hw || !params || !table || !out) return XMC_EINVAL;
    if (N < 1 || pool_bytes < 16 || (pool_bytes & 15)) return XMC_EINVAL;
    if (B < 1 || S < 8 || (S % 8) || S > S_MAX) return XMC_ESHAPE;
    if ((int64_t)B * (S / ROWS) > INT32_MAX) return XMC_ESHAPE;
    if ((reinterpret_cast<uintptr_t>(pool) & 15) || (reinterpret_cast<uintptr_t>(out) & 15)) return XMC_EALIGN;
    if ((reinterpret_cast<uintptr_t>(offsets) & 7) || (reinterpret_cast<uintptr_t>(hw) & 3) || (reinterpret_cast<uintptr_t>(params) & 3) ||
        (reinterpret_cast<uintptr_t>(table) & 3))
        return XMC_EALIGN;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t lds = ((size_t)ROWS * row_units(S) + 1) * 16 + 256 * sizeof(float);
    const dim3 grid(B * (S / ROWS)), block(NT);
    hipLaunchKernelGGL(crop_flip_normalize_kernel, grid, block, lds, st, reinterpret_cast<const uint4*>(pool), pool_bytes / 16, offsets, hw, N,
                       params, table, out, S);
    xmc_note_kernel("crop_flip_normalize_kernel");
    XMC_LAUNCH_CHECK();
    return 0;
}
