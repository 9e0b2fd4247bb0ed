// The text side of a training step from device-resident tables of cached caption embeddings (not in the reference as device code): the three
// tensors a frozen text encoder returns for a batch -- words_embs [B,E,T], sent_embs [B,E], mask [B,T] -- as ONE transposing gather.
//
//   r = rows[b], n = lens[r]
//   words[b][e][t] = t < n ? tok_tab[(tok_offsets[r] + t) * E + e] : 0        sent[b][e] = sent_tab[r * E + e]        mask[b][t] = t >= n
//
// The tables hold the encoder's f32 outputs and the kernel does no arithmetic on a value: the result EQUALS what the encoder returned when
// the cache was built.  Only the valid tokens are stored (token rows of caption r: [lens[r], E] at row tok_offsets[r]).
//
// Access pattern.  A workgroup takes one caption and one chunk of CH = 64 channels.  Its share of words_embs is the CONTIGUOUS run of
// w * T floats at ((b * E + e0) * T), w = min(64, E - e0): 16-byte aligned (E % 4 == 0, e0 % 64 == 0) and a whole number of float4s for
// every T (w % 4 == 0).  Stage in: the n row segments of w floats are read with 16-byte loads, 16 rows per pass of the 256 threads, and
// put into an LDS tile [t][STRIDE].  Write out: consecutive lanes write consecutive float4s of the run; element (e, t) of a float4 comes
// out of the tile at t * STRIDE + e, zero for t >= n.  STRIDE = 65 dwords: `ds_write_b32` / `ds_read_b32` bank on (address / 4) % 32 per
// 32-lane half, so the tile's rows are one bank apart (a stride of 64 would put a whole column on ONE bank: the transposed reads would
// serialise T / 4 deep).  With 65 the bank of element (t, e) is (t + e) % 32; what is left is 2-way on both sides (stage-in: lanes c and
// c + 8 of a row, which step by 4 dwords; write-out: lanes at (t, e) and (t - 4, e + 4), or t and t + 32 at T = 64), on 5 KB of LDS
// traffic per workgroup at T = 20.  No atomics, no inline assembly; the only stores are
// vector stores to the three outputs.
//
// Bounds.  The caller (ops.caption_gather) validates `rows` on the host before it launches.  Independently of that, the kernel clamps the
// row to [0, N), the length to [0, T] and every token row to [0, tok_rows), so no `rows` vector -- and no index file -- can make it read
// outside the tables; its writes depend on (b, e, t) alone.
#include "common.h"

namespace {
constexpr int NT = 256;
constexpr int CH = 64;             // channels per workgroup
constexpr int T_MAX = 64;          // SBERT_ENCODER's cap on TEXT.MAX_LENGTH
constexpr int STRIDE = CH + 1;     // dwords per tile row

__global__ void __launch_bounds__(NT) caption_gather_kernel(const float* __restrict__ sent_tab, const float* __restrict__ tok_tab, int64_t tok_rows,
                                                            const int64_t* __restrict__ tok_offsets, const int32_t* __restrict__ lens, int N,
                                                            const int32_t* __restrict__ rows, int E, int T, int chunks,
                                                            float* __restrict__ words, float* __restrict__ sent, uint8_t* __restrict__ mask) {
    __shared__ float tile[T_MAX * STRIDE];            // 16.6 KB
    const int b = blockIdx.x / chunks, e0 = (blockIdx.x - b * chunks) * CH;
    const int w = min(CH, E - e0), w4 = w >> 2;       // this chunk's channels (a multiple of 4)
    int r = rows[b];
    r = r < 0 ? 0 : (r >= N ? N - 1 : r);
    int n = lens[r];
    n = n < 0 ? 0 : (n > T ? T : n);
    const int64_t first = tok_offsets[r];

    for (int i = threadIdx.x; i < n * (CH / 4); i += NT) {
        const int t = i >> 4, c = i & 15;
        if (c < w4) {
            int64_t row = first + t;
            row = row < 0 ? 0 : (row >= tok_rows ? tok_rows - 1 : row);
            const float4 v = *reinterpret_cast<const float4*>(tok_tab + (size_t)row * E + e0 + 4 * c);
            float* d = tile + t * STRIDE + 4 * c;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
    }
    __syncthreads();

    float4* out = reinterpret_cast<float4*>(words + ((size_t)b * E + e0) * T);
    for (int j = threadIdx.x; j < w4 * T; j += NT) {
        int e = (4 * j) / T, t = 4 * j - e * T;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = t < n ? tile[t * STRIDE + e] : 0.0f;
            if (++t == T) { t = 0; ++e; }
        }
        out[j] = make_float4(v[0], v[1], v[2], v[3]);
    }
    if (threadIdx.x < w4)
        reinterpret_cast<float4*>(sent + (size_t)b * E + e0)[threadIdx.x] =
            reinterpret_cast<const float4*>(sent_tab + (size_t)r * E + e0)[threadIdx.x];
    if (e0 == 0 && threadIdx.x < T) mask[(size_t)b * T + threadIdx.x] = threadIdx.x >= n ? 1 : 0;
}
}  // namespace

extern "C" int xmc_caption_gather(const float* sent_tab, const float* tok_tab, int64_t tok_rows, const int64_t* tok_offsets, const int32_t* lens,
                                  int N, const int32_t* rows, int B, int E, int T, float* words, float* sent, uint8_t* mask, void* stream) {
    if (!sent_tab || !tok_tab || !tok_offsets || !lens || !rows || !words || !sent || !mask) return XMC_EINVAL;
    if (N < 1 || tok_rows < 1) return XMC_EINVAL;
    if (B < 1 || E < 4 || (E % 4) || T < 1 || T > T_MAX) return XMC_ESHAPE;
    const int chunks = (E + CH - 1) / CH;
    if ((int64_t)B * chunks > INT32_MAX) return XMC_ESHAPE;
    if ((reinterpret_cast<uintptr_t>(sent_tab) & 15) || (reinterpret_cast<uintptr_t>(tok_tab) & 15) || (reinterpret_cast<uintptr_t>(words) & 15) ||
        (reinterpret_cast<uintptr_t>(sent) & 15))
        return XMC_EALIGN;
    if ((reinterpret_cast<uintptr_t>(tok_offsets) & 7) || (reinterpret_cast<uintptr_t>(lens) & 3) || (reinterpret_cast<uintptr_t>(rows) & 3))
        return XMC_EALIGN;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(B * chunks), block(NT);
    hipLaunchKernelGGL(caption_gather_kernel, grid, block, 0, st, sent_tab, tok_tab, tok_rows, tok_offsets, lens, N, rows, E, T, chunks, words,
                       sent, mask);
    xmc_note_kernel("caption_gather_kernel");
    XMC_LAUNCH_CHECK();
    return 0;
}
