// Improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) on feature rows
// (xmc_gan_amd/manifold.py): k-nearest-neighbour statistics whose N x N distance matrix is never stored.  Everything is f32.
//
//   d2(a, b) = max(|a|^2 + |b|^2 - 2 a.b, 0).  The dot products are a 128 x 128 block of v_mfma_f32_32x32x2_f32 tiles (2 x 2 per wave, four
//   waves), both operands staged through LDS 32 columns of D at a time, D never split: every a.b is ONE f32 fma chain over D in a fixed
//   order of the columns (inside a group of 8 columns: 0 4 1 5 2 6 3 7 -- the lanes of a half-wave read four consecutive columns with one
//   16-byte LDS read), the same for every pair, every grid and every slice count.  A D that is no multiple of 32 ends with zero columns,
//   which leave the chain's value as it is.
//   The QUERIES are on the MFMA's column dimension: lane l of a wave owns query l & 31 of a 32 x 32 tile and receives 16 candidates' dot
//   products for it in its 16 accumulator registers (rows (r & 3) + 8 (r >> 2) + 4 (l >> 5)).  So the running count, the running minimum
//   and the sorted list of the k smallest are registers of that lane; the loop over the candidates has no cross-lane traffic.  A value is
//   compared with the current k-th first and inserted (a branch-free max/min ladder) only when it is smaller.
//   The four partial states of a query -- two half-waves, two waves -- meet once, through LDS, when the workgroup's candidate range is done.
//   Candidate rows past N carry the norm +inf (their d2 is +inf: in no list, no count, no minimum); query rows past N are not written;
//   in knn_radius2 the pair (i, i) is replaced by +inf by index.
//   slices > 1: gridDim.y workgroups share a query block, each over a range of whole 128-row chunks, and write partial results to `ws`;
//   a second, small launch merges them.  Sums of integers, minima and "the k smallest of a union" are the same whatever the split.
#include <math.h>

#include "common.h"

namespace {
typedef __attribute__((ext_vector_type(16))) float f32x16;
constexpr int NT = 256, TQ = 128, TC = 128, DK = 32, LS = DK + 4;      // LS: LDS row stride (floats): 16-byte reads of 16 rows hit 64 banks once
// slices == 0: as many slices as keep the grid within ONE round of resident workgroups: 256 CUs x 2 (every instantiation fits twice per CU by
// registers and LDS).  A grid a few workgroups above that runs a second round for the stragglers: 47 query blocks x 11 slices = 517 measured
// 9.6 ms for the four calls at N = 6 000, D = 2048, where x 10 = 470 takes one round and 6.6 ms.
constexpr int MAX_SLICES = 64, RESIDENT_WG = 512;

// thread's share of a [128 rows][32 columns] tile: four 16-byte units (8 per row), zero outside the matrix
__device__ __forceinline__ void tile_fetch(const float* __restrict__ x, int N, int D, int row0, int d0, int tid, f32x4 (&v)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = tid + j * NT, row = row0 + (e >> 3), d = d0 + 4 * (e & 7);
        v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (row < N && d < D) v[j] = *reinterpret_cast<const f32x4*>(x + (size_t)row * D + d);
    }
}
__device__ __forceinline__ void tile_store(float* s, int tid, const f32x4 (&v)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = tid + j * NT;
        *reinterpret_cast<f32x4*>(s + (e >> 3) * LS + 4 * (e & 7)) = v[j];
    }
}

// l[] ascending; v < l[KL-1]: v goes in, the largest drops out.  The first KL - k entries are -inf and stay (v > -inf), so l[KL-1] is the
// k-th smallest of what was inserted
template <int KL>
__device__ __forceinline__ void list_insert(float (&l)[KL], float v) {
#pragma unroll
    for (int i = KL - 1; i > 0; --i) l[i] = fmaxf(l[i - 1], fminf(v, l[i]));
    l[0] = fminf(v, l[0]);
}
template <int KL>
__device__ __forceinline__ void list_init(float (&l)[KL], int k) {
#pragma unroll
    for (int i = 0; i < KL; ++i) l[i] = i < KL - k ? -INFINITY : INFINITY;
}

// MODE 0: r2 / ws get the k smallest d2 per query, the pair (i, i) left out (q == c).  MODE 1: count / near2.
template <int MODE, int KL>
__global__ void __launch_bounds__(NT) manifold_kernel(const float* __restrict__ q, const float* __restrict__ qn2, const float* __restrict__ c,
                                                     const float* __restrict__ cn2, const float* __restrict__ cr2, float* __restrict__ r2,
                                                     int32_t* __restrict__ count, float* __restrict__ near2, float* __restrict__ ws, int Nq,
                                                     int Nc, int D, int k, int chunks) {
    __shared__ __attribute__((aligned(16))) float smem[(TQ + TC) * LS];
    __shared__ __attribute__((aligned(16))) float sCn[TC], sCr[TC];
    float* sQ = smem;
    float* sC = smem + TQ * LS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wq = wave & 1, wc = wave >> 1, r = lane & 31, h = lane >> 5;
    const int q0 = blockIdx.x * TQ, s = blockIdx.y, S = gridDim.y;
    const int chunk_lo = (int)((int64_t)s * chunks / S), chunk_hi = (int)((int64_t)(s + 1) * chunks / S);

    int qi[2];
    float qn[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        qi[t] = q0 + wq * 64 + t * 32 + r;
        qn[t] = qi[t] < Nq ? qn2[qi[t]] : 0.f;
    }
    float lst[2][KL];
    int cnt[2] = {0, 0};
    float mn[2] = {INFINITY, INFINITY};
    list_init<KL>(lst[0], k);
    list_init<KL>(lst[1], k);

    const int nd = (D + DK - 1) / DK;
    for (int chunk = chunk_lo; chunk < chunk_hi; ++chunk) {
        const int c0 = chunk * TC;
        __syncthreads();                                   // the previous chunk's epilogue has read sCn / sCr
        if (tid < TC) {
            const int g = c0 + tid;
            sCn[tid] = g < Nc ? cn2[g] : INFINITY;
            if (MODE == 1) sCr[tid] = (g < Nc && cr2) ? cr2[g] : -1.f;
        }
        f32x16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
        f32x4 fq[4], fc[4];
        tile_fetch(q, Nq, D, q0, 0, tid, fq);
        tile_fetch(c, Nc, D, c0, 0, tid, fc);
        for (int ds = 0; ds < nd; ++ds) {
            __syncthreads();                               // everyone is done with the tile in LDS
            tile_store(sQ, tid, fq);
            tile_store(sC, tid, fc);
            __syncthreads();
            if (ds + 1 < nd) {                             // the next tile travels while this one is multiplied
                tile_fetch(q, Nq, D, q0, (ds + 1) * DK, tid, fq);
                tile_fetch(c, Nc, D, c0, (ds + 1) * DK, tid, fc);
            }
#pragma unroll
            for (int t8 = 0; t8 < DK / 8; ++t8) {
                f32x4 av[2], bv[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    av[t] = *reinterpret_cast<const f32x4*>(sC + (wc * 64 + t * 32 + r) * LS + 8 * t8 + 4 * h);
                    bv[t] = *reinterpret_cast<const f32x4*>(sQ + (wq * 64 + t * 32 + r) * LS + 8 * t8 + 4 * h);
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
        // epilogue of the chunk: 2 x 2 tiles x 16 candidates for each of the lane's two queries
#pragma unroll
        for (int tq = 0; tq < 2; ++tq)
#pragma unroll
            for (int tc = 0; tc < 2; ++tc)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int base = wc * 64 + tc * 32 + 8 * g + 4 * h;          // the chunk's row of register 4 g
                    const f32x4 nb = *reinterpret_cast<const f32x4*>(sCn + base);
                    f32x4 rb = {0.f, 0.f, 0.f, 0.f};
                    if (MODE == 1) rb = *reinterpret_cast<const f32x4*>(sCr + base);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float v = fmaxf(fmaf(-2.f, acc[tq][tc][4 * g + e], qn[tq] + nb[e]), 0.f);
                        if (MODE == 0) {
                            if (c0 + base + e == qi[tq]) v = INFINITY;
                            if (v < lst[tq][KL - 1]) list_insert<KL>(lst[tq], v);
                        } else {
                            cnt[tq] += v <= rb[e] ? 1 : 0;
                            mn[tq] = fminf(mn[tq], v);
                        }
                    }
                }
    }

    // the four partial states of a query (part = 2 wc + h) meet in LDS; thread t < 128 finishes query q0 + t
    __syncthreads();
    int* smi = reinterpret_cast<int*>(smem);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int slot = (wq * 64 + t * 32 + r) * 4 + wc * 2 + h;
        if (MODE == 0) {
#pragma unroll
            for (int i = 0; i < KL; ++i) smem[slot * KL + i] = lst[t][i];
        } else {
            smem[slot] = mn[t];
            smi[TQ * 4 + slot] = cnt[t];
        }
    }
    __syncthreads();
    const int qg = q0 + tid;
    if (tid >= TQ || qg >= Nq) return;
    if (MODE == 0) {
        float m[KL];
        list_init<KL>(m, k);
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int i = 0; i < KL; ++i) {
                if (i < KL - k) continue;
                const float v = smem[(tid * 4 + p) * KL + i];
                if (v < m[KL - 1]) list_insert<KL>(m, v);
            }
        if (S == 1) {
            r2[qg] = m[KL - 1];
        } else {
            float* o = ws + ((size_t)s * Nq + qg) * k;
#pragma unroll
            for (int i = 0; i < KL; ++i)
                if (i >= KL - k) o[i - (KL - k)] = m[i];
        }
    } else {
        int n = 0;
        float lo = INFINITY;
        for (int p = 0; p < 4; ++p) {
            n += smi[TQ * 4 + tid * 4 + p];
            lo = fminf(lo, smem[tid * 4 + p]);
        }
        if (S == 1) {
            if (cr2) count[qg] = n;
            if (near2) near2[qg] = lo;
        } else {
            reinterpret_cast<int32_t*>(ws)[(size_t)s * Nq + qg] = n;
            ws[(size_t)(S + s) * Nq + qg] = lo;
        }
    }
}

template <int KL>
__global__ void __launch_bounds__(NT) knn_merge_kernel(const float* __restrict__ ws, float* __restrict__ r2, int N, int k, int S) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= N) return;
    float m[KL];
    list_init<KL>(m, k);
    for (int s = 0; s < S; ++s) {
        const float* p = ws + ((size_t)s * N + i) * k;
        for (int j = 0; j < k; ++j) {
            const float v = p[j];
            if (v < m[KL - 1]) list_insert<KL>(m, v);
        }
    }
    r2[i] = m[KL - 1];
}

__global__ void __launch_bounds__(NT) count_merge_kernel(const float* __restrict__ ws, int32_t* __restrict__ count, float* __restrict__ near2, int N,
                                                        int S) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= N) return;
    int n = 0;
    float lo = INFINITY;
    for (int s = 0; s < S; ++s) {
        n += reinterpret_cast<const int32_t*>(ws)[(size_t)s * N + i];
        lo = fminf(lo, ws[(size_t)(S + s) * N + i]);
    }
    if (count) count[i] = n;
    if (near2) near2[i] = lo;
}

constexpr int SQ_WAVES = NT / 64;
__global__ void __launch_bounds__(NT) row_sqnorm_kernel(const float* __restrict__ x, float* __restrict__ n2, int N, int D) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * SQ_WAVES + (threadIdx.x >> 6);
    if (row >= N) return;                                  // (whole waves)
    const f32x4* __restrict__ p = reinterpret_cast<const f32x4*>(x + (size_t)row * D);
    float acc = 0.f;
    for (int u = lane; u < (D >> 2); u += 64) {
        const f32x4 t = p[u];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = fmaf(t[e], t[e], acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) n2[row] = acc;
}

inline bool bad_dims(int D) { return D < 4 || D % 4 != 0 || D > 4096; }
inline bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
constexpr int MAX_ROWS = 1 << 30;
}  // namespace

extern "C" int xmc_manifold_slices(int Nq, int Nc, int slices) {
    if (Nq < 1 || Nc < 1) return 0;
    const int chunks = (Nc + TC - 1) / TC, qb = (Nq + TQ - 1) / TQ;
    int S = slices > 0 ? slices : RESIDENT_WG / qb;
    if (S > chunks) S = chunks;
    if (S > MAX_SLICES) S = MAX_SLICES;
    return S < 1 ? 1 : S;
}

extern "C" int xmc_row_sqnorm(const float* x, float* n2, int N, int D, void* stream) {
    if (!x || !n2 || N < 1) return XMC_EINVAL;
    if (bad_dims(D) || N > MAX_ROWS) return XMC_ESHAPE;
    if (misaligned16(x) || misaligned16(n2)) return XMC_EALIGN;
    hipLaunchKernelGGL(row_sqnorm_kernel, dim3((N + SQ_WAVES - 1) / SQ_WAVES), dim3(NT), 0, reinterpret_cast<hipStream_t>(stream), x, n2, N, D);
    xmc_note_kernel("row_sqnorm_kernel");
    XMC_LAUNCH_CHECK();
    return 0;
}

extern "C" int xmc_knn_radius2(const float* x, const float* n2, float* r2, float* ws, int64_t ws_bytes, int N, int D, int k, int slices,
                               void* stream) {
    if (!x || !n2 || !r2 || N < 1 || k < 1 || k > 16 || slices < 0) return XMC_EINVAL;
    if (bad_dims(D) || N < k + 1 || N > MAX_ROWS) return XMC_ESHAPE;
    if (misaligned16(x) || misaligned16(n2) || misaligned16(r2) || misaligned16(ws)) return XMC_EALIGN;
    const int S = xmc_manifold_slices(N, N, slices);
    if (S > 1 && (!ws || ws_bytes < (int64_t)S * N * k * (int64_t)sizeof(float))) return XMC_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((N + TQ - 1) / TQ, S), block(NT);
    const int chunks = (N + TC - 1) / TC, KL = k <= 4 ? 4 : k <= 8 ? 8 : 16;
#define XMC_KNN_GO(KL_)                                                                                                                          \
    do {                                                                                                                                         \
        hipLaunchKernelGGL((manifold_kernel<0, KL_>), grid, block, 0, st, x, n2, x, n2, (const float*)nullptr, r2, (int32_t*)nullptr,           \
                           (float*)nullptr, ws, N, N, D, k, chunks);                                                                             \
        XMC_LAUNCH_CHECK();                                                                                                                      \
        if (S > 1) hipLaunchKernelGGL((knn_merge_kernel<KL_>), dim3((N + NT - 1) / NT), block, 0, st, ws, r2, N, k, S);                          \
    } while (0)
    if (KL == 4) XMC_KNN_GO(4); else if (KL == 8) XMC_KNN_GO(8); else XMC_KNN_GO(16);
#undef XMC_KNN_GO
    xmc_note_kernel("manifold_kernel<0, %d>", KL);
    XMC_LAUNCH_CHECK();
    return 0;
}

extern "C" int xmc_manifold_count(const float* a, const float* na2, const float* b, const float* nb2, const float* rb2, int32_t* count,
                                  float* near2, void* ws, int64_t ws_bytes, int Na, int Nb, int D, int slices, void* stream) {
    if (!a || !na2 || !b || !nb2 || Na < 1 || Nb < 1 || slices < 0) return XMC_EINVAL;
    if ((!rb2 && !near2) || (rb2 && !count)) return XMC_EINVAL;
    if (bad_dims(D) || Na > MAX_ROWS || Nb > MAX_ROWS) return XMC_ESHAPE;
    if (misaligned16(a) || misaligned16(na2) || misaligned16(b) || misaligned16(nb2) || misaligned16(rb2) || misaligned16(near2) || misaligned16(ws))
        return XMC_EALIGN;
    if (reinterpret_cast<uintptr_t>(count) & 3) return XMC_EALIGN;
    const int S = xmc_manifold_slices(Na, Nb, slices);
    if (S > 1 && (!ws || ws_bytes < (int64_t)S * Na * 8)) return XMC_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((Na + TQ - 1) / TQ, S), block(NT);
    const int chunks = (Nb + TC - 1) / TC;
    int32_t* cnt = rb2 ? count : nullptr;
    hipLaunchKernelGGL((manifold_kernel<1, 1>), grid, block, 0, st, a, na2, b, nb2, rb2, (float*)nullptr, cnt, near2, reinterpret_cast<float*>(ws), Na,
                       Nb, D, 1, chunks);
    XMC_LAUNCH_CHECK();
    if (S > 1)
        hipLaunchKernelGGL(count_merge_kernel, dim3((Na + NT - 1) / NT), block, 0, st, reinterpret_cast<const float*>(ws), cnt, near2, Na, S);
    xmc_note_kernel("manifold_kernel<1, 1>");
    XMC_LAUNCH_CHECK();
    return 0;
}
