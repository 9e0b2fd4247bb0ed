// Kernel Inception Distance (Binkowski et al. 2018) and Inception Score (Salimans et al. 2016) on feature rows
// (xmc_gan_amd/manifold.py `kid` / `kid_subsets`, xmc_gan_amd/fid.py `InceptionScore`).
//
// poly_mmd: the three kernel sums of the unbiased MMD^2 estimate, k(x, y) = (x.y / D + 1)^3, for all subsets in one launch.
//   A workgroup owns one 128 x 128 tile of one Gram matrix of one subset: 2 x 2 v_mfma_f32_32x32x2_f32 tiles per wave, four waves, both
//   operands staged through LDS 32 columns of D at a time, D never split -- the structure and the fma chain order of manifold_kernel
//   (csrc/manifold.hip), so an element's dot product is the same bits in every tile and for both orders of a pair.  The rows of a tile
//   are GATHERED while they are staged: thread t fetches the 16-byte units of subset positions (t >> 3) + 32 j, whose bank rows it reads
//   from the index table once; a row is D contiguous floats, so no gathered copy of a subset is ever written.
//   Tiles of a subset (T = ceil(m / 128), U = T (T + 1) / 2): [0, U) the upper tiles (ti <= tj) of real x real, [U, 2 U) of
//   generated x generated, [2 U, 2 U + T^2) all tiles of real x generated.  A within-set Gram is symmetric element by element, so its
//   lower tiles are not computed: poly_mmd_merge_kernel counts a strictly upper tile twice.
//   Epilogue: t = fmaf(dot, 1/D, 1), t*t*t in f32, widened to f64, added to the lane's f64 sum in a fixed order; positions >= m and, in
//   a diagonal tile of a within-set Gram, row position == column position are left out.  The lanes meet in a fixed xor butterfly, the
//   four waves in LDS in order, the tile's sum goes to ws[s][tile]; a second launch adds a sum's tiles in order.  No atomics, no tickets.
//
// inception_score: p = softmax(logits row) in f64; per part of consecutive rows H = sum p log p and P[y] = sum p.  A wave owns a row, lane l
//   the classes l, l + 64, ...; their exponentials and the lane's share of P stay in registers (C <= 1024: 16 each).
#include <math.h>

#include "common.h"

namespace {
typedef __attribute__((ext_vector_type(16))) float f32x16;
constexpr int NT = 256, TM = 128, DK = 32, LS = DK + 4;               // LS: LDS row stride (floats), as in manifold.hip
constexpr int MAX_M = 1 << 20, MAX_S = 65535;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// thread's share of a gathered [128 positions][32 columns] tile: four 16-byte units; rowp[j] is the bank row of position (tid >> 3) + 32 j,
// NULL for a position past the subset
__device__ __forceinline__ void gather_fetch(const float* const (&rowp)[4], int D, int d0, int tid, f32x4 (&v)[4]) {
    const int d = d0 + 4 * (tid & 7);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (rowp[j] && d < D) v[j] = *reinterpret_cast<const f32x4*>(rowp[j] + d);
    }
}
__device__ __forceinline__ void gather_store(float* s, int tid, const f32x4 (&v)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4*>(s + ((tid >> 3) + 32 * j) * LS + 4 * (tid & 7)) = v[j];
}

__global__ void __launch_bounds__(NT) poly_mmd_kernel(const float* __restrict__ real, const float* __restrict__ fake,
                                                     const int32_t* __restrict__ idx_real, const int32_t* __restrict__ idx_fake,
                                                     double* __restrict__ ws, int Nr, int Nf, int D, int m, int T, float inv_d) {
    __shared__ __attribute__((aligned(16))) float smem[2 * TM * LS];
    __shared__ double sW[NT / 64];
    float* sB = smem;                 // the tile's columns (the MFMA's B operand)
    float* sA = smem + TM * LS;       // the tile's rows
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wq = wave & 1, wc = wave >> 1, r = lane & 31, h = lane >> 5;
    const int s = blockIdx.y, U = T * (T + 1) / 2;
    int p = blockIdx.x, kind = 2, ti, tj;                  // kind 0: real x real, 1: generated x generated, 2: real x generated
    if (p < 2 * U) {
        kind = p >= U ? 1 : 0;
        int u = p - kind * U;
        ti = 0;
        while (u >= T - ti) {
            u -= T - ti;
            ++ti;
        }
        tj = ti + u;
    } else {
        p -= 2 * U;
        ti = p / T;
        tj = p - ti * T;
    }
    const float* __restrict__ bankA = kind == 1 ? fake : real;
    const float* __restrict__ bankB = kind == 0 ? real : fake;
    const int32_t* __restrict__ ixA = (kind == 1 ? idx_fake : idx_real) + (size_t)s * m;
    const int32_t* __restrict__ ixB = (kind == 0 ? idx_real : idx_fake) + (size_t)s * m;
    const int NA = kind == 1 ? Nf : Nr, NB = kind == 0 ? Nr : Nf;
    const int a0 = ti * TM, b0 = tj * TM;

    const float* rowA[4];
    const float* rowB[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int pa = a0 + (tid >> 3) + 32 * j, pb = b0 + (tid >> 3) + 32 * j;
        rowA[j] = rowB[j] = nullptr;
        if (pa < m) rowA[j] = bankA + (size_t)min(max(ixA[pa], 0), NA - 1) * D;      // (the caller checked the table; the clamp keeps a
        if (pb < m) rowB[j] = bankB + (size_t)min(max(ixB[pb], 0), NB - 1) * D;      // wrong one inside the bank)
    }

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
    const int nd = (D + DK - 1) / DK;
    f32x4 fa[4], fb[4];
    gather_fetch(rowA, D, 0, tid, fa);
    gather_fetch(rowB, D, 0, tid, fb);
    for (int ds = 0; ds < nd; ++ds) {
        __syncthreads();                               // everyone is done with the tile in LDS
        gather_store(sA, tid, fa);
        gather_store(sB, tid, fb);
        __syncthreads();
        if (ds + 1 < nd) {                             // the next tile travels while this one is multiplied
            gather_fetch(rowA, D, (ds + 1) * DK, tid, fa);
            gather_fetch(rowB, D, (ds + 1) * DK, tid, fb);
        }
#pragma unroll
        for (int t8 = 0; t8 < DK / 8; ++t8) {
            f32x4 av[2], bv[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                av[t] = *reinterpret_cast<const f32x4*>(sA + (wc * 64 + t * 32 + r) * LS + 8 * t8 + 4 * h);
                bv[t] = *reinterpret_cast<const f32x4*>(sB + (wq * 64 + t * 32 + r) * LS + 8 * t8 + 4 * h);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int tq = 0; tq < 2; ++tq)
#pragma unroll
                    for (int tc = 0; tc < 2; ++tc)
                        acc[tq][tc] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tc][e], bv[tq][e], acc[tq][tc], 0, 0, 0);
        }
    }

    // the lane holds column position b0 + wq*64 + tq*32 + r and, in register 4 g + e, row position a0 + wc*64 + tc*32 + 8 g + 4 h + e
    const bool diag = kind != 2 && ti == tj;
    double sum = 0.0;
#pragma unroll
    for (int tq = 0; tq < 2; ++tq) {
        const int pb = b0 + wq * 64 + tq * 32 + r;
#pragma unroll
        for (int tc = 0; tc < 2; ++tc)
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int pa = a0 + wc * 64 + tc * 32 + 8 * g + 4 * h + e;
                    const float t = fmaf(acc[tq][tc][4 * g + e], inv_d, 1.f);
                    const float k3 = t * t * t;
                    const bool in = pa < m && pb < m && !(diag && pa == pb);
                    sum += in ? (double)k3 : 0.0;
                }
    }
    sum = wave_sum_f64(sum);
    if (lane == 0) sW[wave] = sum;
    __syncthreads();
    if (tid == 0) ws[(size_t)s * gridDim.x + blockIdx.x] = ((sW[0] + sW[1]) + sW[2]) + sW[3];
}

// out[s][kind]: the tiles of a sum in order; a strictly upper tile of a within-set Gram stands for its mirror image too
__global__ void __launch_bounds__(NT) poly_mmd_merge_kernel(const double* __restrict__ ws, double* __restrict__ out, int S, int T) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= 3 * S) return;
    const int s = i / 3, kind = i - 3 * s, U = T * (T + 1) / 2, P = 2 * U + T * T;
    const double* __restrict__ w = ws + (size_t)s * P;
    double sum = 0.0;
    if (kind == 2) {
        for (int t = 0; t < T * T; ++t) sum += w[2 * U + t];
    } else {
        int u = kind * U;
        for (int ti = 0; ti < T; ++ti)
            for (int tj = ti; tj < T; ++tj, ++u) sum += tj == ti ? w[u] : 2.0 * w[u];
    }
    out[i] = sum;
}

// ---- inception score
constexpr int IS_ROWS = 64, IS_WAVES = NT / 64, IS_MAX_C = 1024, IS_PER_LANE = IS_MAX_C / 64;

__host__ __device__ inline int is_part_lo(int s, int N, int splits) { return (int)((int64_t)s * N / splits); }
inline int is_groups(int N, int splits) { return ((N + splits - 1) / splits + IS_ROWS - 1) / IS_ROWS; }       // a part has at most ceil(N / splits) rows

// ws [splits][G][C + 1]: P partials, then H
__global__ void __launch_bounds__(NT) inception_score_kernel(const float* __restrict__ logits, int64_t ld, double* __restrict__ ws, int N, int C,
                                                            int splits) {
    __shared__ double sP[IS_WAVES][IS_MAX_C];
    __shared__ double sH[IS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, s = blockIdx.y, g = blockIdx.x, G = gridDim.x;
    const int lo = is_part_lo(s, N, splits), hi = is_part_lo(s + 1, N, splits);
    double pl[IS_PER_LANE];
#pragma unroll
    for (int j = 0; j < IS_PER_LANE; ++j) pl[j] = 0.0;
    double hsum = 0.0;
    for (int i = 0; i < IS_ROWS / IS_WAVES; ++i) {
        const int row = lo + g * IS_ROWS + wave * (IS_ROWS / IS_WAVES) + i;
        if (row >= hi) break;                              // (whole waves)
        const float* __restrict__ x = logits + (size_t)row * ld;
        double v[IS_PER_LANE];
        double mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < IS_PER_LANE; ++j) {
            const int y = lane + 64 * j;
            v[j] = y < C ? (double)x[y] : -INFINITY;
            mx = fmax(mx, v[j]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
        double z = 0.0;
#pragma unroll
        for (int j = 0; j < IS_PER_LANE; ++j) {
            const int y = lane + 64 * j;
            v[j] -= mx;                                    // x - max <= 0
            z += y < C ? exp(v[j]) : 0.0;
        }
        z = wave_sum_f64(z);
        const double lz = log(z), iz = 1.0 / z;
        double hr = 0.0;
#pragma unroll
        for (int j = 0; j < IS_PER_LANE; ++j) {
            const int y = lane + 64 * j;
            if (y < C) {
                const double pj = exp(v[j]) * iz;
                pl[j] += pj;
                hr += pj > 0.0 ? pj * (v[j] - lz) : 0.0;   // p log p -> 0 as p -> 0
            }
        }
        hsum += wave_sum_f64(hr);
    }
#pragma unroll
    for (int j = 0; j < IS_PER_LANE; ++j) sP[wave][lane + 64 * j] = pl[j];
    if (lane == 0) sH[wave] = hsum;
    __syncthreads();
    double* __restrict__ o = ws + ((size_t)s * G + g) * (C + 1);
    for (int y = tid; y < C; y += NT) o[y] = ((sP[0][y] + sP[1][y]) + sP[2][y]) + sP[3][y];
    if (tid == 0) o[C] = ((sH[0] + sH[1]) + sH[2]) + sH[3];
}

__global__ void __launch_bounds__(NT) inception_score_merge_kernel(const double* __restrict__ ws, double* __restrict__ H, double* __restrict__ P,
                                                                  int C, int G, int splits) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= splits * (C + 1)) return;
    const int s = i / (C + 1), y = i - s * (C + 1);
    double sum = 0.0;
    for (int g = 0; g < G; ++g) sum += ws[((size_t)s * G + g) * (C + 1) + y];
    if (y == C) H[s] = sum; else P[(size_t)s * C + y] = sum;
}

inline bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
}  // namespace

extern "C" int xmc_poly_mmd_tiles(int m) {
    if (m < 1 || m > MAX_M) return 0;
    const int T = (m + TM - 1) / TM;
    return T * (T + 1) + T * T;
}

extern "C" int xmc_poly_mmd_sums(const float* real, const float* fake, const int32_t* idx_real, const int32_t* idx_fake, double* out, double* ws,
                                 int64_t ws_bytes, int Nr, int Nf, int D, int S, int m, void* stream) {
    if (!real || !fake || !idx_real || !idx_fake || !out || !ws || Nr < 1 || Nf < 1 || S < 1 || S > MAX_S) return XMC_EINVAL;
    if (D < 4 || D % 4 != 0 || D > 4096 || m < 2 || m > MAX_M) return XMC_ESHAPE;
    if (misaligned(real, 16) || misaligned(fake, 16) || misaligned(idx_real, 4) || misaligned(idx_fake, 4) || misaligned(out, 8) || misaligned(ws, 8))
        return XMC_EALIGN;
    const int T = (m + TM - 1) / TM, P = xmc_poly_mmd_tiles(m);
    if (ws_bytes < (int64_t)S * P * (int64_t)sizeof(double)) return XMC_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(poly_mmd_kernel, dim3(P, S), dim3(NT), 0, st, real, fake, idx_real, idx_fake, ws, Nr, Nf, D, m, T, 1.0f / (float)D);
    XMC_LAUNCH_CHECK();
    hipLaunchKernelGGL(poly_mmd_merge_kernel, dim3((3 * S + NT - 1) / NT), dim3(NT), 0, st, ws, out, S, T);
    xmc_note_kernel("poly_mmd_kernel");
    XMC_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t xmc_inception_score_ws_bytes(int N, int C, int splits) {
    if (N < 1 || N > (1 << 30) || C < 1 || C > IS_MAX_C || splits < 1 || splits > N) return 0;
    return (int64_t)splits * is_groups(N, splits) * (C + 1) * (int64_t)sizeof(double);
}

extern "C" int xmc_inception_score(const float* logits, int64_t ld, double* H, double* P, double* ws, int64_t ws_bytes, int N, int C, int splits,
                                   void* stream) {
    if (!logits || !H || !P || !ws || N < 1 || splits < 1 || splits > N || ld < C) return XMC_EINVAL;
    if (C < 1 || C > IS_MAX_C || N > (1 << 30)) return XMC_ESHAPE;
    if (misaligned(logits, 4) || misaligned(H, 8) || misaligned(P, 8) || misaligned(ws, 8)) return XMC_EALIGN;
    if (splits > MAX_S || ws_bytes < xmc_inception_score_ws_bytes(N, C, splits)) return XMC_EINVAL;
    const int G = is_groups(N, splits);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(inception_score_kernel, dim3(G, splits), dim3(NT), 0, st, logits, ld, ws, N, C, splits);
    XMC_LAUNCH_CHECK();
    hipLaunchKernelGGL(inception_score_merge_kernel, dim3((splits * (C + 1) + NT - 1) / NT), dim3(NT), 0, st, ws, H, P, C, G, splits);
    xmc_note_kernel("inception_score_kernel");
    XMC_LAUNCH_CHECK();
    return 0;
}
