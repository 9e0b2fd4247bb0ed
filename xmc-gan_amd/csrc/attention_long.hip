// Attention for sequences of up to 1024 tokens, exact f32 on the MFMA (CLIP ViT-B/16 and L/14 at 197 / 257 / 577 tokens, CLIP's own
// text context of 77): softmax(Q K^T / sqrt(64) + mask) V per (sample, head) from the fused projection f32 [B*T, 3H], rows [Q | K | V],
// the layout xmc_attention_short reads.  Forward only, f32 only, every output element has one writer and a fixed summation order.
//
//   One workgroup = two waves = 64 queries of one (sample, head); a wave owns 32 of them for the whole kernel.  K and V are streamed
//   through LDS in tiles of 64 keys, so LDS use does not depend on T.
//
//   Both products are v_mfma_f32_32x32x2_f32 with the QUERY on the MFMA's column dimension (as manifold.hip holds its queries):
//     S^T = K Q^T   A = K (key l & 31, channel pair from LDS), B = Q^T (query l & 31; the wave's 32 x 64 block of Q, pre-scaled by
//                   0.125, stays in 32 registers).  Lane l receives in accumulator register r the score of query l & 31 and key
//                   (r & 3) + 8 (r >> 2) + 4 (l >> 5) of a 32-key half tile: a query's running maximum and sum are per-lane registers
//                   plus one exchange between lanes l and l ^ 32.
//     O^T = V^T P^T B = P^T needs key k of the pair on lanes 32 k .. 32 k + 31 with the query on l & 31 -- which is what register r of
//                   the score accumulator already holds, for the key pair ((r & 3) + 8 (r >> 2), the same + 4).  So A = V^T is read
//                   from LDS in that key order (row kr + 4 (l >> 5), channel l & 31) and P never goes through LDS.  The output
//                   accumulators (two 32-channel tiles) hold channel (r & 3) + 8 (r >> 2) + 4 (l >> 5) of query l & 31: the rescale by
//                   exp(m_old - m_new) is a per-lane scalar, and four registers are 16 consecutive output bytes.
//
//   Keys in sight of query r of sample b: j < len_b, and j <= r when causal.  Scores out of sight are excluded from the maximum and
//   enter the sum and the second product as exact zeros; staged K / V rows >= len_b and Q rows >= len_b are zero-filled and never
//   read, so nothing non-finite can form and the bytes of a sample do not depend on T, on the batch, or on what lies behind its length.
//   The maximum starts at -FLT_MAX (finite); key 0 is in sight of every valid query, so it is a real score after the first tile.
//   Key tiles wholly behind len_b or, when causal, behind the query block's last row are skipped: the trip count is uniform per
//   workgroup.  Inside a tile, a wave passes over the second 32-key half when none of its keys is in sight of any of the wave's queries
//   (the 5 keys of the last tile at T = 197, the diagonal tile of a causal block's first wave): every value there is an exact zero,
//   so the bytes are those of the full tile.  A wave none of whose 32 queries is valid (the second wave of a 1-row tail block at T = 257) only helps staging.
#include <cfloat>
#include "encoder_kernels.h"

namespace {

constexpr int AL_MAX_T = 1024;      // ATTENTION_LONG_MAX_T
constexpr int AL_QB = 64;           // queries per workgroup (32 per wave)
constexpr int AL_KT = 64;           // keys per LDS tile
constexpr int AL_KS = AT_D + 4;     // K row stride: 16-byte row reads by 32 lanes of different keys
constexpr int AL_VS = AT_D + 8;     // V row stride: rows kr and kr + 4 read by the two half-waves fall into different banks (4 * 72 = 32 mod 64)
typedef __attribute__((ext_vector_type(16))) float f32x16;

template <bool CAUSAL>
__global__ __launch_bounds__(128) void attention_long_kernel(const float* __restrict__ qkv, const int32_t* __restrict__ lens,
                                                             float* __restrict__ out, int T, int H, int nqb) {
    __shared__ __attribute__((aligned(16))) float k_s[AL_KT][AL_KS];
    __shared__ __attribute__((aligned(16))) float v_s[AL_KT][AL_VS];
    const int b = blockIdx.x / nqb, qb = blockIdx.x % nqb, head = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lq = lane & 31, hh = lane >> 5;
    const int len = lens ? min(max(lens[b], 0), T) : T;
    const float* base = qkv + (size_t)b * T * 3 * H + head * AT_D;
    const int q = qb * AL_QB + wave * 32 + lq;                 // this lane's query row
    const bool wave_on = qb * AL_QB + wave * 32 < len;         // wave-uniform: any valid query in the wave
    // key tiles in sight of the block: keys < len, and <= the block's last row when causal (uniform per workgroup)
    const int kend = CAUSAL ? min(len, qb * AL_QB + AL_QB) : len;
    const int ntiles = (kend + AL_KT - 1) / AL_KT;
    // the same bound for the wave's 32 queries: a 32-key half tile wholly behind it holds exact zeros for every lane and is passed over
    const int wend = CAUSAL ? min(len, qb * AL_QB + wave * 32 + 32) : len;

    // Q of the lane's query, scaled by 1 / sqrt(64) (a power of two: exact), channels 8 g + 4 hh + c in qr[g][c]
    f32x4 qr[8];
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        qr[g] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (q < len) qr[g] = *reinterpret_cast<const f32x4*>(base + (size_t)q * 3 * H + 8 * g + 4 * hh) * 0.125f;
    }
    f32x16 o0, o1;                                             // channels [0, 32) and [32, 64) of the query
#pragma unroll
    for (int r = 0; r < 16; ++r) o0[r] = 0.f, o1[r] = 0.f;
    float m = -FLT_MAX, l = 0.f;                               // running maximum (shared by the lane pair) and this lane's half of the sum

    for (int kt = 0; kt < ntiles; ++kt) {
        const int k0 = kt * AL_KT;
        __syncthreads();                                       // the previous tile has been read
        for (int i = tid; i < AL_KT * (AT_D / 4); i += 128) {
            const int t = i / (AT_D / 4), c = (i % (AT_D / 4)) * 4;
            f32x4 kv = f32x4{0.f, 0.f, 0.f, 0.f}, vv = kv;
            if (k0 + t < len) {
                const float* r = base + (size_t)(k0 + t) * 3 * H + c;
                kv = *reinterpret_cast<const f32x4*>(r + H), vv = *reinterpret_cast<const f32x4*>(r + 2 * H);
            }
            *reinterpret_cast<f32x4*>(&k_s[t][c]) = kv;
            *reinterpret_cast<f32x4*>(&v_s[t][c]) = vv;
        }
        __syncthreads();
        if (!wave_on) continue;                                // (wave-uniform; the barriers above are reached by every wave)
        const bool half1 = k0 + 32 < wend;                     // (wave-uniform) keys k0 + 32 .. k0 + 63: any in sight of the wave?

        // scores of the lane's query against the tile's two 32-key halves
        f32x16 s0, s1;
#pragma unroll
        for (int r = 0; r < 16; ++r) s0[r] = 0.f, s1[r] = 0.f;
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const f32x4 ka = *reinterpret_cast<const f32x4*>(&k_s[lq][8 * g + 4 * hh]);
#pragma unroll
            for (int c = 0; c < 4; ++c) s0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[c], qr[g][c], s0, 0, 0, 0);
        }
        if (half1) {
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const f32x4 kb = *reinterpret_cast<const f32x4*>(&k_s[32 + lq][8 * g + 4 * hh]);
#pragma unroll
                for (int c = 0; c < 4; ++c) s1 = __builtin_amdgcn_mfma_f32_32x32x2f32(kb[c], qr[g][c], s1, 0, 0, 0);
            }
        }
        // the keys in sight of this query: below `lim`
        const int lim = CAUSAL ? min(len, q + 1) : len;
        float tm = -FLT_MAX;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kj = k0 + (r & 3) + 8 * (r >> 2) + 4 * hh;
            if (kj < lim) tm = fmaxf(tm, s0[r]);
            if (kj + 32 < lim) tm = fmaxf(tm, s1[r]);
        }
        tm = fmaxf(tm, __shfl_xor(tm, 32));
        const float mn = fmaxf(m, tm);
        const float alpha = expf(m - mn);                      // first tile: exp(-FLT_MAX - mn) = 0 on a zero accumulator
        m = mn;
        float ps = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kj = k0 + (r & 3) + 8 * (r >> 2) + 4 * hh;
            s0[r] = kj < lim ? expf(s0[r] - mn) : 0.f;         // out of sight: excluded
        }
        if (half1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int kj = k0 + 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                s1[r] = kj < lim ? expf(s1[r] - mn) : 0.f;
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) ps += s0[r];
#pragma unroll
        for (int r = 0; r < 16; ++r) ps += s1[r];
        l = l * alpha + ps;
#pragma unroll
        for (int r = 0; r < 16; ++r) o0[r] *= alpha, o1[r] *= alpha;
        // O^T += V^T P^T: register r of the scores is the key pair (kr, kr + 4) of one MFMA
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kr = (r & 3) + 8 * (r >> 2) + 4 * hh;
            o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v_s[kr][lq], s0[r], o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v_s[kr][32 + lq], s0[r], o1, 0, 0, 0);
        }
        if (half1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int kr = 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v_s[kr][lq], s1[r], o0, 0, 0, 0);
                o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v_s[kr][32 + lq], s1[r], o1, 0, 0, 0);
            }
        }
    }

    if (q >= T) return;
    // the two halves of the sum, added in the same order on both lanes of the pair
    const float lo = __shfl(l, lq), hi = __shfl(l, lq + 32);
    const float den = lo + hi;
    const bool valid = q < len;                                // rows of padded queries: zero, as the short kernel writes them
    float* orow = out + ((size_t)b * T + q) * H + head * AT_D + 4 * hh;
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
        f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f}, c = a;
        if (valid) {
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = o0[4 * rg + i] / den, c[i] = o1[4 * rg + i] / den;
        }
        *reinterpret_cast<f32x4*>(orow + 8 * rg) = a;
        *reinterpret_cast<f32x4*>(orow + 32 + 8 * rg) = c;
    }
}

}  // namespace

extern "C" int xmc_attention_long(const float* qkv, const int32_t* lens, float* out, int B, int T, int heads, int head_dim, int causal,
                                  void* stream) {
    if (!qkv || !out) return XMC_EINVAL;
    if (B < 1 || heads < 1 || heads > 65535 || T < 1 || T > AL_MAX_T || head_dim != AT_D) return XMC_ESHAPE;
    const int nqb = (T + AL_QB - 1) / AL_QB;
    if ((int64_t)B * nqb > 0x7fffffff) return XMC_ESHAPE;
    if (!aligned16(qkv) || !aligned16(out) || !aligned4(lens)) return XMC_EALIGN;
    const dim3 grid((unsigned)(B * nqb), (unsigned)heads), blk(128);
    if (causal)
        hipLaunchKernelGGL(attention_long_kernel<true>, grid, blk, 0, (hipStream_t)stream, qkv, lens, out, T, heads * AT_D, nqb);
    else
        hipLaunchKernelGGL(attention_long_kernel<false>, grid, blk, 0, (hipStream_t)stream, qkv, lens, out, T, heads * AT_D, nqb);
    xmc_note_kernel("attention_long_kernel<%s>", causal ? "true" : "false");
    XMC_LAUNCH_CHECK();
    return 0;
}
