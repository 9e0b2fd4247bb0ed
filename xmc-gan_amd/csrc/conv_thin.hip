// Convolution whose SOURCE has 8 stored channels (an image: 3 channels padded to 8), unit stride, bf16 -- the discriminator's
// first layer (df_gan.py:130 `conv_img`, 3 -> ndf) and the data gradient of the generator's last layer (df_gan.py:86-90,
// ngf <- 3).  The generic implicit-GEMM kernel spends one 64-byte K sub-step per tap on 16 bytes of data and re-gathers every
// pixel nine times (measured 29 TFLOP/s, 4x the HBM time of the layer); this kernel is built for what the layer is, a stream:
//
//   * a persistent workgroup walks 8x32-pixel output tiles; the (8+2)x(32+2) source patch is 5.4 KB of LDS;
//   * K = taps x 8 channels: one 16-byte unit of a pixel IS one lane's 8 K-values of a 16x16x32 MFMA operand, so a 3x3 kernel
//     is three MFMA K-steps (taps 0-3, 4-7, 8 + zero weights) whose pixel operand is a single ds_read_b128 at the tap-shifted
//     patch position; the weights (<= 12 fragments) stay in registers for the life of the workgroup;
//   * MFMA roles as in conv_tile.hip's ptile3: A = weight rows (permuted while loading), B = pixels, so each lane ends up with
//     BN/4 consecutive output channels of one pixel and stores 16-byte units straight from registers.
// HBM traffic = source once (+6 % halo) + destination once.
#include "common.h"
#include "conv_plan.h"
#include <stdlib.h>

namespace {

struct ThinCfg {
    int tiles_y, tiles_x, PW, PH, dh0, dw0;
};

template <int BN>
__global__ __launch_bounds__(256) void thin_in_kernel(const XmcConvDesc d, const ThinCfg t, int ntiles) {
    constexpr int TH = 8, TW = 32, TN = BN / 16, UPL = BN / 32, KS = 3;
    __shared__ __attribute__((aligned(16))) unsigned char patch[(TH + 4) * (TW + 4) * 16];
    const int tid = threadIdx.x, lane = tid & 63, wm = tid >> 6;
    const int fr = lane & 15, fc = lane >> 4;
    const int PW = t.PW, PH = t.PH, dh0 = t.dh0, dw0 = t.dw0;
    const u32x4* __restrict__ src16 = reinterpret_cast<const u32x4*>(d.src);
    const u32x4* __restrict__ w16 = reinterpret_cast<const u32x4*>(d.wpk);

    // weights -> registers.  K-step ks, lane group fc <-> tap 4*ks + fc; physical row (j, q) <-> channel (q/4)*(BN/4) + j*4 + q%4
    u32x4 wf[KS][TN];
    int toff[KS];                                 // byte offset of this lane's tap in the patch, per K-step
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int tap = ks * 4 + fc;
        const bool live = tap < d.ntaps;
        const int tt = live ? tap : 0;
        toff[ks] = ((d.dh[0][tt] - dh0) * PW + (d.dw[0][tt] - dw0)) * 16;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int lrow = (fr >> 2) * (BN / 4) + j * 4 + (fr & 3);
            wf[ks][j] = live ? w16[(size_t)d.wi[0][tt] * d.CDw + lrow] : u32x4{0, 0, 0, 0};
        }
    }
    // patch staging: thread -> up to 2 patch pixels; halo bits as in ptile3 (1 top, 2 bottom, 4 left, 8 right)
    int ppix[2], psrc[2];
    unsigned halo[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int pp = tid + it * 256;
        const int py = pp / PW, px = pp - py * PW;
        const bool in = pp < PH * PW;
        ppix[it] = in ? pp : -1;
        psrc[it] = in ? (dh0 + py) * d.SW + (dw0 + px) : 0;
        halo[it] = !in ? 0u : ((py < -dh0 ? 1u : 0u) | (py >= TH - dh0 ? 2u : 0u) | (px < -dw0 ? 4u : 0u) | (px >= TW - dw0 ? 8u : 0u));
    }
    int pbase[4], eoff[4];
    const int cd8 = d.CD / 8;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = wm * 2 + (i >> 1), c = (i & 1) * 16 + fr;
        pbase[i] = (r * PW + c) * 16;
        eoff[i] = (r * d.DW + c) * cd8 + fc * UPL;
    }
    const int ch0 = fc * (BN / 4);
    float bias8[UPL][8];
#pragma unroll
    for (int u = 0; u < UPL; ++u)
#pragma unroll
        for (int c = 0; c < 8; ++c) bias8[u][c] = (d.bias && ch0 + u * 8 < d.CD) ? d.bias[ch0 + u * 8 + c] : 0.f;
    const float slope = d.act == XMC_ACT_LRELU ? XMC_LRELU : 1.f;
    const int tpi = t.tiles_y * t.tiles_x;
    bf16x8* __restrict__ dst8 = reinterpret_cast<bf16x8*>(d.dst);
    const bf16x8* __restrict__ mask8 = reinterpret_cast<const bf16x8*>(d.mask);
    const float pscale = d.pool_scale == 0.f ? 0.25f : d.pool_scale;

    u32x4 pv[2];
    unsigned okbits = 0;
    auto issue = [&](int tile) {
        const int img = tile / tpi, trem = tile - img * tpi;
        const int ty = trem / t.tiles_x, tx = trem - ty * t.tiles_x;
        const int a0 = ty * TH, b0 = tx * TW;
        const int base = (img * d.SH + a0) * d.SW + b0;
        const unsigned border = (a0 + dh0 < 0 ? 1u : 0u) | (a0 + PH + dh0 > d.SH ? 2u : 0u) | (b0 + dw0 < 0 ? 4u : 0u) | (b0 + PW + dw0 > d.SW ? 8u : 0u);
        okbits = 0;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const bool ok = (halo[it] & border) == 0;
            pv[it] = src16[(unsigned)(base + (ok ? psrc[it] : 0))];
            okbits |= ok ? (1u << it) : 0u;
        }
    };
    const XcdWalk xw = xmc_xcd_walk(ntiles);
    int tile = xw.first;
    if (tile < xw.end) issue(tile);
    for (; tile < xw.end; tile += xw.step) {
        const int img = tile / tpi, trem = tile - img * tpi;
        const int ty = trem / t.tiles_x, tx = trem - ty * t.tiles_x;
        __syncthreads();                          // previous tile's reads are done
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            u32x4 v = pv[it];
            if (!((okbits >> it) & 1)) v = u32x4{0, 0, 0, 0};
            if (ppix[it] >= 0) *reinterpret_cast<u32x4*>(patch + ppix[it] * 16) = v;
        }
        __syncthreads();
        if (tile + xw.step < xw.end) issue(tile + xw.step);
        const int dbase = ((img * d.DH + ty * TH) * d.DW + tx * TW) * cd8;
        // pixel blocks i and i+2 are vertical neighbours (rows 2*wm and 2*wm+1, same columns) of the same lane: they are
        // finished together so that the optional third output (2x2 average of the rounded result, XmcConvDesc.dst_pool) is a
        // sum of two registers plus one exchange with lane ^ 1
#pragma unroll
        for (int ip = 0; ip < 2; ++ip) {
            float fin[2][UPL][8];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int i = ip + 2 * h;
                f32x4 acc[TN];
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const u32x4 pf = *reinterpret_cast<const u32x4*>(patch + pbase[i] + toff[ks]);
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[j] = XMC_MFMA_16x16x32(__builtin_bit_cast(bf16x8, wf[ks][j]), __builtin_bit_cast(bf16x8, pf), acc[j], 0, 0, 0);
                }
#pragma unroll
                for (int u = 0; u < UPL; ++u) {
                    if (ch0 + u * 8 >= d.CD) continue;
                    bf16x8 o;
                    if (mask8 == nullptr) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const float x0 = acc[2 * u][q] + bias8[u][q], x1 = acc[2 * u + 1][q] + bias8[u][4 + q];
                            o[q] = (xmc_h16)fmaxf(x0, x0 * slope);
                            o[4 + q] = (xmc_h16)fmaxf(x1, x1 * slope);
                        }
                    } else {              // data gradient of the layer above a LeakyReLU: times LeakyReLU'(mask), mask in the dst layout
                        const bf16x8 mk = mask8[dbase + eoff[i] + u];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const float x0 = acc[2 * u][q] + bias8[u][q], x1 = acc[2 * u + 1][q] + bias8[u][4 + q];
                            o[q] = (xmc_h16)xmc_pin_f32(fmaxf(x0, x0 * slope) * lrelu_slope((float)mk[q]));          // pinned: gtail_bwd_kernel
                            o[4 + q] = (xmc_h16)xmc_pin_f32(fmaxf(x1, x1 * slope) * lrelu_slope((float)mk[4 + q]));  // promises these bits
                        }
                    }
                    dst8[dbase + eoff[i] + u] = o;
#pragma unroll
                    for (int q = 0; q < 8; ++q) fin[h][u][q] = (float)o[q];
                }
            }
            if (d.dst_pool) {
                bf16x8* __restrict__ pool8 = reinterpret_cast<bf16x8*>(d.dst_pool);
                const int prow = ty * (TH / 2) + wm, pcol = tx * (TW / 2) + ((ip * 16 + fr) >> 1);
#pragma unroll
                for (int u = 0; u < UPL; ++u) {
                    if (ch0 + u * 8 >= d.CD) continue;
                    bf16x8 o;
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        float sm = fin[0][u][q] + fin[1][u][q];
                        sm += xmc_xor1(sm);
                        o[q] = (xmc_h16)(pscale * sm);
                    }
                    if ((fr & 1) == 0) pool8[((img * (d.DH >> 1) + prow) * (d.DW >> 1) + pcol) * cd8 + fc * UPL + u] = o;
                }
            }
        }
    }
}

// ---- The backward of the generator's tail (LeakyReLU -> conv_out 32 -> 3 -> tanh, df_gan.py:84-88) as ONE pass over its 32-channel
// activation y (ops.GBlockEndFn.backward).  thin_in_kernel<32> as conv_out's data gradient already holds, per tile, both
// operands of conv_out's WEIGHT gradient: the (8+2)x(32+2) patch of its source dpre = dy * tanh'(img) in LDS and, for the mask of
// its epilogue, y at exactly the tile's pixels.  Written over the positions q of y,
//     dW[tap][co][ci] = sum_q y[q][ci] * dpre[q + (dh, dw)(tap)][co]          ((dh, dw)(tap): the data gradient's own tap shift)
// needs no halo of y, and the patch's zero padding supplies the border terms.  So this kernel
//   * stages dpre itself from dy and img (xmc_tanh_bwd's arithmetic and rounding, applied to the 16-byte unit on its way into LDS:
//     dpre is never written), then runs thin_in_kernel<32>'s MFMAs, mask, stores and 2x2 sum pool unchanged: dz and dsc come out
//     bit-identical;
//   * WG: each wave passes the y units of its 2 x 16 pixels per half-tile through 3 KB of LDS of its own and reads them back pixel-
//     major (ds_read_b64_tr_b16, as conv_wgrad.hip) as the B operand of a [12 tap slots x 4 channels] x [32 ci] x [32 pixels] product,
//     whose A operand is the same transposing read on the patch at the tap-shifted pixel (the first 8 bytes of a pixel: conv_out has
//     <= 4 output channels); 24 accumulator registers per lane live across the persistent tile loop, the four waves meet in LDS
//     at the end and the workgroup issues 1152 f32 atomics into the packed buffer of the weight-gradient kernels.  The bias
//     gradient is the sum of the centre tap's A fragments;
//   * takes a partial last tile in x (any even W), which the unfused kernel declines.
constexpr int GT_YSTR = 96;          // bytes per pixel of the y image: 64 + 32, the transposing reads of a 32-lane half then cover all banks once
// Registers: WG needs 138 (no scratch) -> 3 workgroups per CU.  Bound to 4 per CU it spills one register and, at grids equal to what is
// resident (1024 / 768 workgroups), runs no faster (0.593 / 0.598 ms at 256 x 256x256); a grid beyond the resident set costs 20 %.
template <bool WG>
__global__ __launch_bounds__(256, WG ? 3 : 4) void gtail_bwd_kernel(const XmcConvDesc d, const u32x4* __restrict__ img16, float* __restrict__ dwp,
                                                        float* __restrict__ dbias, int dw_rows, int tiles_y, int tiles_x, int ntiles) {
    constexpr int TH = 8, TW = 32, PW = TW + 2, PH = TH + 2, KS = 3, TN = 2, NRED = 9 * 4 * 32;
    __shared__ __attribute__((aligned(16))) unsigned char patch[PH * PW * 16];
    __shared__ __attribute__((aligned(16))) unsigned char ylds[WG ? 4 * 32 * GT_YSTR : 16];
    static_assert(!WG || 4 * 32 * GT_YSTR >= NRED * 4, "the cross-wave reduction reuses the y image");
    const int tid = threadIdx.x, lane = tid & 63, wm = tid >> 6;
    const int fr = lane & 15, fc = lane >> 4;
    const u32x4* __restrict__ dy16 = reinterpret_cast<const u32x4*>(d.src);
    const u32x4* __restrict__ w16 = reinterpret_cast<const u32x4*>(d.wpk);

    // data-gradient weights -> registers, exactly as thin_in_kernel<32> (K-step ks, lane group fc <-> tap 4*ks + fc)
    u32x4 wf[KS][TN];
    int toff[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int tap = ks * 4 + fc;
        const bool live = tap < 9;
        const int tt = live ? tap : 0;
        toff[ks] = ((d.dh[0][tt] + 1) * PW + (d.dw[0][tt] + 1)) * 16;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int lrow = (fr >> 2) * 8 + j * 4 + (fr & 3);
            wf[ks][j] = live ? w16[(size_t)d.wi[0][tt] * d.CDw + lrow] : u32x4{0, 0, 0, 0};
        }
    }
    // patch staging: thread -> up to 2 patch pixels
    int ppix[2], ppy[2], ppx[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int pp = tid + it * 256;
        ppy[it] = pp / PW; ppx[it] = pp - ppy[it] * PW;
        ppix[it] = pp < PH * PW ? pp : -1;
    }
    int pbase[4], eoff[4];
    const int cd8 = 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = wm * 2 + (i >> 1), c = (i & 1) * 16 + fr;
        pbase[i] = (r * PW + c) * 16;
        eoff[i] = (r * d.DW + c) * cd8 + fc;
    }
    // weight gradient: lane 4q + pp of a 16-lane group addresses K row (pixel) 4*fc + q [+16], 4 elements of column block pp
    const int tq = fr >> 2, tp = fr & 3;
    int aoff[3];                                  // A: tap slot tp of row block j <-> tap 4j + tp (slots of taps >= 9: any valid address, rows dropped)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int tap = 4 * j + tp < 9 ? 4 * j + tp : 0;
        aoff[j] = ((wm * 2 + d.dh[0][tap] + 1) * PW + (4 * fc + tq + d.dw[0][tap] + 1)) * 16;
    }
    unsigned char* const ywave = ylds + (WG ? wm * 32 * GT_YSTR : 0);
    const int ywr = fr * GT_YSTR + fc * 16;                     // + h * 16 rows: this lane's unit of pixel (row h, column fr) of the half-tile
    const int yrd = (4 * fc + tq) * GT_YSTR + tp * 8;           // + 32 bytes per 16-channel block, + 16 rows for the second half of the K step
    f32x4 accw[3][2];
#pragma unroll
    for (int j = 0; j < 3; ++j) accw[j][0] = accw[j][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;

    const int tpi = tiles_y * tiles_x;
    bf16x8* __restrict__ dst8 = reinterpret_cast<bf16x8*>(d.dst);
    const bf16x8* __restrict__ mask8 = reinterpret_cast<const bf16x8*>(d.mask);
    const float pscale = d.pool_scale == 0.f ? 0.25f : d.pool_scale;

    u32x4 pvd[2], pvi[2];
    auto issue = [&](int tile) {
        const int img = tile / tpi, trem = tile - img * tpi;
        const int ty = trem / tiles_x, tx = trem - ty * tiles_x;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int gy = ty * TH - 1 + ppy[it], gx = tx * TW - 1 + ppx[it];
            const bool ok = ppix[it] >= 0 && (unsigned)gy < (unsigned)d.SH && (unsigned)gx < (unsigned)d.SW;
            const unsigned idx = ok ? (unsigned)((img * d.SH + gy) * d.SW + gx) : 0u;
            const u32x4 z = {0, 0, 0, 0};
            pvd[it] = ok ? dy16[idx] : z;
            pvi[it] = ok ? img16[idx] : z;
        }
    };
    const XcdWalk xw = xmc_xcd_walk(ntiles);
    int tile = xw.first;
    if (tile < xw.end) issue(tile);
    for (; tile < xw.end; tile += xw.step) {
        const int img = tile / tpi, trem = tile - img * tpi;
        const int ty = trem / tiles_x, tx = trem - ty * tiles_x;
        __syncthreads();                          // previous tile's reads are done
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const bf16x8 a = __builtin_bit_cast(bf16x8, pvd[it]), b = __builtin_bit_cast(bf16x8, pvi[it]);
            bf16x8 v;
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = (xmc_h16)tanh_bwd_f((float)a[k], (float)b[k]);      // (0, 0) outside the image -> 0
            if (ppix[it] >= 0) *reinterpret_cast<bf16x8*>(patch + ppix[it] * 16) = v;
        }
        __syncthreads();
        if (tile + xw.step < xw.end) issue(tile + xw.step);
        const int dbase = ((img * d.DH + ty * TH) * d.DW + tx * TW) * cd8;
#pragma unroll
        for (int ip = 0; ip < 2; ++ip) {
            const bool colok = tx * TW + ip * 16 + fr < d.DW;        // partial last tile in x
            bf16x8 mk[2], fin[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int i = ip + 2 * h;
                f32x4 acc[TN];
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const u32x4 pf = *reinterpret_cast<const u32x4*>(patch + pbase[i] + toff[ks]);
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[j] = XMC_MFMA_16x16x32(__builtin_bit_cast(bf16x8, wf[ks][j]), __builtin_bit_cast(bf16x8, pf), acc[j], 0, 0, 0);
                }
                const bf16x8 zero8 = __builtin_bit_cast(bf16x8, u32x4{0, 0, 0, 0});
                mk[h] = colok ? mask8[dbase + eoff[i]] : zero8;
                bf16x8 o;
#pragma unroll
                for (int q = 0; q < 4; ++q) {       // thin_in_kernel's epilogue with no bias and no activation (acc + 0: -0 -> +0 as there)
                    const float x0 = acc[0][q] + 0.f, x1 = acc[1][q] + 0.f;
                    o[q] = (xmc_h16)xmc_pin_f32(x0 * lrelu_slope((float)mk[h][q]));
                    o[4 + q] = (xmc_h16)xmc_pin_f32(x1 * lrelu_slope((float)mk[h][4 + q]));
                }
                if (colok) dst8[dbase + eoff[i]] = o;
                fin[h] = o;
            }
            if (d.dst_pool) {
                bf16x8* __restrict__ pool8 = reinterpret_cast<bf16x8*>(d.dst_pool);
                const int prow = ty * (TH / 2) + wm, pcol = tx * (TW / 2) + ((ip * 16 + fr) >> 1);
                bf16x8 o;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    float sm = (float)fin[0][q] + (float)fin[1][q];
                    sm += xmc_xor1(sm);
                    o[q] = (xmc_h16)(pscale * sm);
                }
                if ((fr & 1) == 0 && colok) pool8[((img * (d.DH >> 1) + prow) * (d.DW >> 1) + pcol) * cd8 + fc] = o;
            }
            if constexpr (WG) {
                // K step = the 32 pixels (rows 2*wm, 2*wm + 1) x (columns 16*ip .. +15) this wave just finished; all 64 lanes take part
                // (the transposing reads need EXEC all ones); y of a column beyond the image is 0
                *reinterpret_cast<bf16x8*>(ywave + ywr) = mk[0];
                *reinterpret_cast<bf16x8*>(ywave + ywr + 16 * GT_YSTR) = mk[1];
                __builtin_amdgcn_wave_barrier();
                bf16x8 af[3], bq[2];
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const unsigned char* base = patch + aoff[j] + ip * 16 * 16;
                    const bf16x4 lo = xmc_ds_read_tr16(base), hi = xmc_ds_read_tr16(base + PW * 16);
                    af[j] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                }
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const unsigned char* base = ywave + yrd + i * 32;
                    const bf16x4 lo = xmc_ds_read_tr16(base), hi = xmc_ds_read_tr16(base + 16 * GT_YSTR);
                    bq[i] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                }
#pragma unroll
                for (int j = 0; j < 3; ++j)
#pragma unroll
                    for (int i = 0; i < 2; ++i) accw[j][i] = XMC_MFMA_16x16x32(af[j], bq[i], accw[j][i], 0, 0, 0);
                // bias gradient: slot 0 of row block 1 is the centre tap (4), i.e. dpre at the 32 pixels themselves
#pragma unroll
                for (int k = 0; k < 8; ++k) bsum += (float)af[1][k];
                __builtin_amdgcn_wave_barrier();          // the next half-tile's y units are written after these reads
            }
        }
    }
    if constexpr (WG) {
        // D[row = 4 * slot + co][col = ci]: lane (fr, fc) holds slot fc (tap 4j + fc), co = r, ci = 16 i + fr.  Four waves -> one sum in LDS,
        // then 128-byte rows of atomics into dwp[tap][co][ci] (the layout xmc_unpack_wgrad* reads)
        float* const red = reinterpret_cast<float*>(ylds);
        __syncthreads();
        for (int id = tid; id < NRED; id += 256) red[id] = 0.f;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int tap = 4 * j + fc;
            if (tap < 9) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) atomicAdd(&red[(tap * 4 + r) * 32 + i * 16 + fr], accw[j][i][r]);
            }
        }
        __syncthreads();
        for (int id = tid; id < NRED; id += 256) {
            const int tap = id >> 7, co = (id >> 5) & 3, ci = id & 31;
            atomicAdd(&dwp[((size_t)d.wi[0][tap] * dw_rows + co) * 32 + ci], red[id]);
        }
        if (dbias) {
            float v = tp == fr ? bsum : 0.f;           // lanes fr < 4 of each group: slot 0, channel fr
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            if (lane < 4) atomicAdd(&dbias[(blockIdx.x & (XMC_BIAS_REPLICAS - 1)) * d.CS + lane], v);
        }
    }
}


// 1x1 convolution with few channels (the discriminator's shortcut convolutions on the pooled input, df_gan.py:280,286-291, and
// their data gradients): nothing to stage -- a lane's 16-byte unit of a pixel IS its K-fragment, so the source goes straight
// from global memory into the MFMA B operand (16 pixels x 64 bytes per wave load, fully coalesced), the weights (<= 16
// fragments) live in registers, and the result leaves in 64-byte-per-pixel contiguous stores.  Pure stream: HBM bound.
// By-product for the backward pass of a discriminator block (ops.ResDBwdFn): the kernel that streams `dout` as the SOURCE
// of the shortcut's data gradient also writes `dout x LeakyReLU'(branch)` from the block's sign bits (MASKED: src_masked[unit] =
// src[unit] with the lanes of cleared bits times `slope`, rounded like xmc_signmask_apply) -- the separate mask pass read dout again.
__device__ __forceinline__ u32x4 mask_unit(u32x4 v, unsigned bits, float slope) {
    bf16x8 h = __builtin_bit_cast(bf16x8, v);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float f = (float)h[k];
        h[k] = (xmc_h16)(((bits >> k) & 1u) ? f : slope * f);
    }
    return __builtin_bit_cast(u32x4, h);
}

// SPLIT (round 5, XmcConvDesc.wpk_lo): the weights are the pair hi + lo = round16(w) + round16(w - round16(w)); a second register
// set and a second MFMA per K step into the same accumulator (the launch is bound by its HBM stream, not by its matrix work).
template <int KS, int TN, bool MASKED = false, bool SPLIT = false>   // KS = Cin / 32 K-steps, TN = Cout(padded) / 16 row blocks
__global__ __launch_bounds__(256) void pw1x1_kernel(const XmcConvDesc d, int ngroups, const unsigned char* __restrict__ sbits, u32x4* __restrict__ smasked,
                                                    float mslope) {
    const int lane = threadIdx.x & 63, fr = lane & 15, fc = lane >> 4;
    const int cs_units = d.CS >> 3, cd8 = d.CD >> 3;
    const u32x4* __restrict__ src16 = reinterpret_cast<const u32x4*>(d.src);
    const u32x4* __restrict__ w16 = reinterpret_cast<const u32x4*>(d.wpk);
    bf16x8* __restrict__ dst8 = reinterpret_cast<bf16x8*>(d.dst);
    u32x4 wf[KS][TN], wl[SPLIT ? KS : 1][SPLIT ? TN : 1];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int lrow = (j >> 1) * 32 + (fr >> 2) * 8 + (j & 1) * 4 + (fr & 3);      // see conv_tile.hip: 64-byte stores per pixel
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            wf[ks][j] = w16[((size_t)d.wi[0][0] * d.CDw + lrow) * cs_units + ks * 4 + fc];
            if (SPLIT) wl[ks][j] = reinterpret_cast<const u32x4*>(d.wpk_lo)[((size_t)d.wi[0][0] * d.CDw + lrow) * cs_units + ks * 4 + fc];
        }
    }
    float bias8[TN / 2][8];
#pragma unroll
    for (int u = 0; u < TN / 2; ++u)
#pragma unroll
        for (int c = 0; c < 8; ++c) bias8[u][c] = (d.bias && u * 32 + fc * 8 < d.CD) ? d.bias[u * 32 + fc * 8 + c] : 0.f;
    const float slope = d.act == XMC_ACT_LRELU ? XMC_LRELU : 1.f;
    const int wave_g = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    constexpr int UNR = 4;                     // pixel groups in flight per wave
    for (int g0 = wave_g * UNR; g0 < ngroups; g0 += nwaves * UNR) {
        u32x4 pf[UNR][KS];
#pragma unroll
        for (int r = 0; r < UNR; ++r) {
            const int g = g0 + r < ngroups ? g0 + r : ngroups - 1;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) pf[r][ks] = src16[(size_t)(g * 16 + fr) * cs_units + ks * 4 + fc];
        }
        if (MASKED) {
#pragma unroll
            for (int r = 0; r < UNR; ++r) {
                if (g0 + r >= ngroups) break;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const size_t idx = (size_t)((g0 + r) * 16 + fr) * cs_units + ks * 4 + fc;
                    smasked[idx] = mask_unit(pf[r][ks], sbits[idx], mslope);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < UNR; ++r) {
            if (g0 + r >= ngroups) break;
            f32x4 acc[TN];
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    if (SPLIT) acc[j] = XMC_MFMA_16x16x32(__builtin_bit_cast(bf16x8, wl[ks][j]), __builtin_bit_cast(bf16x8, pf[r][ks]), acc[j], 0, 0, 0);
                    acc[j] = XMC_MFMA_16x16x32(__builtin_bit_cast(bf16x8, wf[ks][j]), __builtin_bit_cast(bf16x8, pf[r][ks]), acc[j], 0, 0, 0);
                }
            const size_t pix = (size_t)(g0 + r) * 16 + fr;
#pragma unroll
            for (int u = 0; u < TN / 2; ++u) {
                if (u * 32 + fc * 8 >= d.CD) continue;
                bf16x8 o;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float x0 = acc[2 * u][q] + bias8[u][q], x1 = acc[2 * u + 1][q] + bias8[u][4 + q];
                    o[q] = (xmc_h16)fmaxf(x0, x0 * slope);
                    o[4 + q] = (xmc_h16)fmaxf(x1, x1 * slope);
                }
                dst8[pix * cd8 + u * 4 + fc] = o;
            }
        }
    }
}

template <int KS, int TN>
int launch_pw(const XmcConvDesc& d, int ngroups, hipStream_t st, const unsigned char* sbits, void* smasked, float mslope) {
    int nb = (ngroups + 4 * 4 - 1) / (4 * 4);           // 4 waves per block, 4 groups per wave and iteration
    if (nb > 256 * 8) nb = 256 * 8;
    if (d.wpk_lo) {      // the pair form, forward: D's 64 -> 128 shortcut, G's 128 -> 64 and 64 -> 32 ones (the wider ones: launch_pww)
        if constexpr ((KS == 2 && TN == 8) || (KS == 4 && TN == 4) || (KS == 2 && TN == 2)) {
            if (smasked) return 1;
            hipLaunchKernelGGL((pw1x1_kernel<KS, TN, false, true>), dim3(nb), dim3(256), 0, st, d, ngroups, nullptr, nullptr, 0.f);
            xmc_note_kernel("pw1x1_kernel<%d, %d, false, true>", KS, TN);
            XMC_LAUNCH_CHECK();
            return 0;
        } else {
            return 1;
        }
    }
    if (smasked) hipLaunchKernelGGL((pw1x1_kernel<KS, TN, true>), dim3(nb), dim3(256), 0, st, d, ngroups, sbits, (u32x4*)smasked, mslope);
    else hipLaunchKernelGGL((pw1x1_kernel<KS, TN, false>), dim3(nb), dim3(256), 0, st, d, ngroups, nullptr, nullptr, 0.f);
    xmc_note_kernel(smasked ? "pw1x1_kernel<%d, %d, true>" : "pw1x1_kernel<%d, %d>", KS, TN);
    XMC_LAUNCH_CHECK();
    return 0;
}

// 1x1 convolution with MANY channels (the learned shortcuts of the deeper discriminator blocks, 128 -> 256 and 256 -> 512, and their
// data gradients): the weights no longer fit in registers, so they sit in LDS -- the workgroup's column slice, staged once, rows
// padded by 16 bytes (16 consecutive rows then cover every bank exactly once per ds_read_b128 of a lane group) -- and everything
// else is pw1x1_kernel: the source goes from global memory straight into the MFMA B operand, four 16-pixel groups in flight per
// wave, each weight fragment read once per 64 pixels, 64-byte-per-pixel stores.  8 waves per workgroup (2 per SIMD) share the
// slice.  85-170 FLOP/byte: an HBM stream (the gather kernel ran these at 1.7-2.6 TB/s: two K steps of prologue and an LDS
// transposition of the result per 256x256 tile).
template <int KS, bool MASKED = false, bool SPLIT = false>   // KS = Cin / 32 K-steps (4 or 8); MASKED: see pw1x1_kernel (the first column slice writes it)
__global__ __launch_bounds__(512) void pw1x1w_kernel(const XmcConvDesc d, int ngroups, int ncols, const unsigned char* __restrict__ sbits,
                                                     u32x4* __restrict__ smasked, float mslope) {
    extern __shared__ __attribute__((aligned(16))) unsigned char wlds[];
    constexpr int RSTR = KS * 64 * (SPLIT ? 2 : 1) + 16;         // bytes per weight row (SPLIT: the row's hi half, then its lo half)
    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, fc = lane >> 4;
    const int cs_units = d.CS >> 3, cd8 = d.CD >> 3;
    const int c0 = blockIdx.y * ncols;         // first output channel of this workgroup's slice
    const u32x4* __restrict__ src16 = reinterpret_cast<const u32x4*>(d.src);
    const u32x4* __restrict__ w16 = reinterpret_cast<const u32x4*>(d.wpk);
    bf16x8* __restrict__ dst8 = reinterpret_cast<bf16x8*>(d.dst);
    // physical row (block j, r) <- logical channel (j/2)*32 + (r/4)*8 + (j%2)*4 + r%4 (conv_tile.hip: lane group fc ends with 8
    // consecutive channels in its two accumulator blocks -> 16-byte stores, 64 bytes per pixel per 32 channels)
    for (int id = tid; id < ncols * KS * 4; id += 512) {
        const int row = id / (KS * 4), ch = id - row * (KS * 4);
        const int j = row >> 4, r = row & 15;
        const int lrow = (j >> 1) * 32 + (r >> 2) * 8 + (j & 1) * 4 + (r & 3);
        *reinterpret_cast<u32x4*>(wlds + row * RSTR + ch * 16) = w16[((size_t)d.wi[0][0] * d.CDw + c0 + lrow) * cs_units + ch];
        if (SPLIT) *reinterpret_cast<u32x4*>(wlds + row * RSTR + KS * 64 + ch * 16) =
                reinterpret_cast<const u32x4*>(d.wpk_lo)[((size_t)d.wi[0][0] * d.CDw + c0 + lrow) * cs_units + ch];
    }
    __syncthreads();
    const float slope = d.act == XMC_ACT_LRELU ? XMC_LRELU : 1.f;
    const int wave_g = blockIdx.x * 8 + (tid >> 6), nwaves = gridDim.x * 8;
    constexpr int UNR = 4;
    const int nu = ncols >> 5;                 // 32-channel units of the slice
    for (int g0 = wave_g * UNR; g0 < ngroups; g0 += nwaves * UNR) {
        u32x4 pf[UNR][KS];
#pragma unroll
        for (int r = 0; r < UNR; ++r) {
            const int g = g0 + r < ngroups ? g0 + r : ngroups - 1;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) pf[r][ks] = src16[(size_t)(g * 16 + fr) * cs_units + ks * 4 + fc];
        }
        if (MASKED && blockIdx.y == 0) {
#pragma unroll
            for (int r = 0; r < UNR; ++r) {
                if (g0 + r >= ngroups) break;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const size_t idx = (size_t)((g0 + r) * 16 + fr) * cs_units + ks * 4 + fc;
                    smasked[idx] = mask_unit(pf[r][ks], sbits[idx], mslope);
                }
            }
        }
        for (int u = 0; u < nu; ++u) {
            f32x4 acc[UNR][2];
#pragma unroll
            for (int r = 0; r < UNR; ++r) acc[r][0] = acc[r][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            const unsigned char* const wr = wlds + (u * 32 + fr) * RSTR + fc * 16;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const bf16x8 wa = *reinterpret_cast<const bf16x8*>(wr + ks * 64), wb = *reinterpret_cast<const bf16x8*>(wr + 16 * RSTR + ks * 64);
                if (SPLIT) {
                    const bf16x8 la = *reinterpret_cast<const bf16x8*>(wr + KS * 64 + ks * 64), lb = *reinterpret_cast<const bf16x8*>(wr + 16 * RSTR + KS * 64 + ks * 64);
#pragma unroll
                    for (int r = 0; r < UNR; ++r) {
                        acc[r][0] = XMC_MFMA_16x16x32(la, __builtin_bit_cast(bf16x8, pf[r][ks]), acc[r][0], 0, 0, 0);
                        acc[r][1] = XMC_MFMA_16x16x32(lb, __builtin_bit_cast(bf16x8, pf[r][ks]), acc[r][1], 0, 0, 0);
                    }
                }
#pragma unroll
                for (int r = 0; r < UNR; ++r) {
                    acc[r][0] = XMC_MFMA_16x16x32(wa, __builtin_bit_cast(bf16x8, pf[r][ks]), acc[r][0], 0, 0, 0);
                    acc[r][1] = XMC_MFMA_16x16x32(wb, __builtin_bit_cast(bf16x8, pf[r][ks]), acc[r][1], 0, 0, 0);
                }
            }
            const int ch = c0 + u * 32 + fc * 8;
            if (ch >= d.CD) continue;
            float b8[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) b8[c] = d.bias ? d.bias[ch + c] : 0.f;
#pragma unroll
            for (int r = 0; r < UNR; ++r) {
                if (g0 + r >= ngroups) break;
                bf16x8 o;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float x0 = acc[r][0][q] + b8[q], x1 = acc[r][1][q] + b8[4 + q];
                    o[q] = (xmc_h16)fmaxf(x0, x0 * slope);
                    o[4 + q] = (xmc_h16)fmaxf(x1, x1 * slope);
                }
                dst8[((size_t)(g0 + r) * 16 + fr) * cd8 + (ch >> 3)] = o;
            }
        }
    }
}

template <int KS>
int launch_pww(const XmcConvDesc& d, int ngroups, hipStream_t st, const unsigned char* sbits, void* smasked, float mslope) {
    // the column slice of a workgroup: as many 32-channel units as fit in LDS, dividing CDw evenly (256 x 512: two slices of 135 KB)
    const bool split = d.wpk_lo != nullptr;
    if (split && smasked) return 1;
    const int RSTR = KS * 64 * (split ? 2 : 1) + 16;
    int ny = 1;
    while ((size_t)(d.CDw / ny) * RSTR > XMC_MAX_DYN_LDS || d.CDw % ny != 0 || (d.CDw / ny) % 32 != 0) {
        if (++ny > d.CDw / 32) return 1;
    }
    const int ncols = d.CDw / ny;
    const size_t lds = (size_t)ncols * RSTR;
    int nb = (ngroups + 8 * 4 - 1) / (8 * 4);           // 8 waves per block, 4 groups per wave and iteration
    if (nb > 256 / ny) nb = 256 / ny;                   // one workgroup per CU (the slice is staged once per workgroup)
    if (nb < 1) nb = 1;
    if (split) {
        XMC_ALLOW_BIG_LDS((pw1x1w_kernel<KS, false, true>));
        hipLaunchKernelGGL((pw1x1w_kernel<KS, false, true>), dim3(nb, ny), dim3(512), lds, st, d, ngroups, ncols, nullptr, nullptr, 0.f);
        xmc_note_kernel("pw1x1w_kernel<%d, false, true>", KS);
        XMC_LAUNCH_CHECK();
        return 0;
    }
    if (smasked) {
        XMC_ALLOW_BIG_LDS((pw1x1w_kernel<KS, true>));
        hipLaunchKernelGGL((pw1x1w_kernel<KS, true>), dim3(nb, ny), dim3(512), lds, st, d, ngroups, ncols, sbits, (u32x4*)smasked, mslope);
    } else {
        XMC_ALLOW_BIG_LDS((pw1x1w_kernel<KS, false>));
        hipLaunchKernelGGL((pw1x1w_kernel<KS, false>), dim3(nb, ny), dim3(512), lds, st, d, ngroups, ncols, nullptr, nullptr, 0.f);
    }
    xmc_note_kernel(smasked ? "pw1x1w_kernel<%d, true>" : "pw1x1w_kernel<%d>", KS);
    XMC_LAUNCH_CHECK();
    return 0;
}

// ---- The entry of a generator block with a learned shortcut (G_Block with in_dim != out_dim, df_gan.py:199-216; ops.GBlockEntryFn,
// DESIGN 4.1): the block input x feeds the affine pair h = lrelu(lrelu(x g0 + b0) g1 + b1) AND the 1x1 shortcut sc = c_sc(x), and in the
// backward both gradients of x meet again.  Two kernels, one per direction, stream x ONCE each:
//   * gentry_fwd_kernel is pw1x1_kernel / pw1x1w_kernel (same MFMA, same channel-to-K mapping, same order of K steps, same epilogue: sc
//     is theirs bit for bit) whose 16-byte units, on their way into the B operand, also pass through affine2_fwd_f and leave as h;
//   * gentry_bwd_kernel forms dskip = c_sc^T dsc per 16-pixel group on the MFMAs (again the 1x1 kernels' arithmetic), rounds it to the
//     storage format -- the value affine2_bwd_kernel reads from memory today -- and hands it through a wave-private LDS slab to the
//     affine backward's own thread-to-unit mapping (a lane owns ONE 8-channel unit of many pixels: 32 parameter and 32 sum registers),
//     which runs affine2_bwd_unit on it: dx, its 2x2 sum pool and the four per-sample sums.  dskip is never written.
// Work: an image is cut into groups of 16 pixels (POOL: four 2x2 quads, so that both rows of a quad are one lane's two steps and its
// two columns are lanes C8 apart); a group never straddles images, a partial last group is masked.  A workgroup owns a contiguous run of
// groups, its waves take them in turn, and each wave keeps its image's parameters (forward: LDS, read per unit; backward: registers)
// and flushes its sums with one set of atomics per image it met.  The grid is the resident set (see gtail_bwd_kernel's note).
struct GEntryArgs {
    const void *x, *dy, *dsc, *wpk;
    void *h, *sc, *dx, *dx_pool;
    const float *bias, *g0, *b0, *g1, *b1;
    float *dg0, *db0, *dg1, *db1;
    int N, H, W, gpi, nvg, per;          // groups per image, N * gpi, groups per workgroup
    float slope;
};

// weight rows -> LDS as pw1x1w_kernel stages its slice (rows padded by 16 bytes; physical row (block j, r) <- logical channel
// (j/2)*32 + (r/4)*8 + (j%2)*4 + r%4), or -> registers as pw1x1_kernel holds them
template <int KS, int TN, bool WLDS, int NW>
__device__ __forceinline__ void gentry_weights(const u32x4* __restrict__ w16, unsigned char* wlds, u32x4 (&wf)[WLDS ? 1 : KS][WLDS ? 1 : TN], int tid, int fr, int fc) {
    constexpr int RSTR = KS * 64 + 16;
    if constexpr (WLDS) {
        for (int id = tid; id < TN * 16 * KS * 4; id += NW * 64) {
            const int row = id / (KS * 4), ch = id - row * (KS * 4);
            const int j = row >> 4, r = row & 15;
            const int lrow = (j >> 1) * 32 + (r >> 2) * 8 + (j & 1) * 4 + (r & 3);
            *reinterpret_cast<u32x4*>(wlds + row * RSTR + ch * 16) = w16[(size_t)lrow * (KS * 4) + ch];
        }
        __syncthreads();
    } else {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int lrow = (j >> 1) * 32 + (fr >> 2) * 8 + (j & 1) * 4 + (fr & 3);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) wf[ks][j] = w16[(size_t)lrow * (KS * 4) + ks * 4 + fc];
        }
    }
}

template <int KS, int TN, bool WLDS, int NW>      // KS = Cin / 32 K-steps, TN = Cout / 16 row blocks, NW waves per workgroup
__global__ __launch_bounds__(NW * 64) void gentry_fwd_kernel(const GEntryArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char glds[];
    constexpr int CIN = KS * 32, C8 = KS * 4, CO8 = TN * 2, UNR = 4;
    constexpr int RSTR = KS * 64 + 16, WBYTES = WLDS ? TN * 16 * RSTR : 0;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, fr = lane & 15, fc = lane >> 4;
    const u32x4* __restrict__ src16 = reinterpret_cast<const u32x4*>(a.x);
    bf16x8* __restrict__ h8 = reinterpret_cast<bf16x8*>(a.h);
    bf16x8* __restrict__ sc8 = reinterpret_cast<bf16x8*>(a.sc);
    float* const par = reinterpret_cast<float*>(glds + WBYTES) + wv * 4 * CIN;          // this wave's image: [g0 | b0 | g1 | b1][CIN]
    u32x4 wf[WLDS ? 1 : KS][WLDS ? 1 : TN];
    gentry_weights<KS, TN, WLDS, NW>(reinterpret_cast<const u32x4*>(a.wpk), glds, wf, tid, fr, fc);
    float bias8[WLDS ? 1 : TN / 2][8];
    if constexpr (!WLDS) {
#pragma unroll
        for (int u = 0; u < TN / 2; ++u)
#pragma unroll
            for (int c = 0; c < 8; ++c) bias8[u][c] = a.bias ? a.bias[u * 32 + fc * 8 + c] : 0.f;
    }
    const float slope = a.slope, one = 1.f;          // `one`: the 1x1 kernels' epilogue fmaxf(v, v * slope) with no activation
    const int HW = a.H * a.W;
    const int lo = blockIdx.x * a.per, hi = min(lo + a.per, a.nvg);
    int cur = -1;
    for (int g0 = lo + wv * UNR; g0 < hi; g0 += NW * UNR) {
        const int n = g0 / a.gpi, gl0 = g0 - n * a.gpi;              // gpi and `per` are multiples of UNR: the UNR groups share the image
        if (n != cur) {
            const float* vec[4] = {a.g0, a.b0, a.g1, a.b1};
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int q = 0; q < 4; ++q)
                for (int c = lane; c < CIN; c += 64) par[q * CIN + c] = vec[q][(size_t)n * CIN + c];
            __builtin_amdgcn_wave_barrier();
            cur = n;
        }
        size_t pix[UNR];
        bool ok[UNR];
        u32x4 pf[UNR][KS];
#pragma unroll
        for (int r = 0; r < UNR; ++r) {
            const int p = (gl0 + r) * 16 + fr;
            ok[r] = p < HW;
            pix[r] = (size_t)n * HW + (ok[r] ? p : HW - 1);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) pf[r][ks] = src16[pix[r] * C8 + ks * 4 + fc];
        }
        // h: the affine pair on every unit this lane holds
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const f32x4* pq = reinterpret_cast<const f32x4*>(par + (ks * 4 + fc) * 8);
            float P[4][8];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 lo4 = pq[q * (CIN / 4)], hi4 = pq[q * (CIN / 4) + 1];
#pragma unroll
                for (int k = 0; k < 4; ++k) { P[q][k] = lo4[k]; P[q][4 + k] = hi4[k]; }
            }
#pragma unroll
            for (int r = 0; r < UNR; ++r) {
                const bf16x8 xv = __builtin_bit_cast(bf16x8, pf[r][ks]);
                bf16x8 o;
#pragma unroll
                for (int k = 0; k < 8; ++k) o[k] = (xmc_h16)affine2_fwd_f((float)xv[k], P[0][k], P[1][k], P[2][k], P[3][k], slope, true);
                if (ok[r]) h8[pix[r] * C8 + ks * 4 + fc] = o;
            }
        }
        // sc: the 1x1 product of the same units
        if constexpr (!WLDS) {
#pragma unroll
            for (int r = 0; r < UNR; ++r) {
                if ((gl0 + r) * 16 >= HW) break;
                f32x4 acc[TN];
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[j] = XMC_MFMA_16x16x32(__builtin_bit_cast(bf16x8, wf[ks][j]), __builtin_bit_cast(bf16x8, pf[r][ks]), acc[j], 0, 0, 0);
#pragma unroll
                for (int u = 0; u < TN / 2; ++u) {
                    bf16x8 o;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float x0 = acc[2 * u][q] + bias8[u][q], x1 = acc[2 * u + 1][q] + bias8[u][4 + q];
                        o[q] = (xmc_h16)fmaxf(x0, x0 * one);
                        o[4 + q] = (xmc_h16)fmaxf(x1, x1 * one);
                    }
                    if (ok[r]) sc8[pix[r] * CO8 + u * 4 + fc] = o;
                }
            }
        } else {
#pragma unroll 1
            for (int u = 0; u < TN / 2; ++u) {
                f32x4 acc[UNR][2];
#pragma unroll
                for (int r = 0; r < UNR; ++r) acc[r][0] = acc[r][1] = f32x4{0.f, 0.f, 0.f, 0.f};
                const unsigned char* const wr = glds + (u * 32 + fr) * RSTR + fc * 16;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const bf16x8 wa = *reinterpret_cast<const bf16x8*>(wr + ks * 64), wb = *reinterpret_cast<const bf16x8*>(wr + 16 * RSTR + ks * 64);
#pragma unroll
                    for (int r = 0; r < UNR; ++r) {
                        acc[r][0] = XMC_MFMA_16x16x32(wa, __builtin_bit_cast(bf16x8, pf[r][ks]), acc[r][0], 0, 0, 0);
                        acc[r][1] = XMC_MFMA_16x16x32(wb, __builtin_bit_cast(bf16x8, pf[r][ks]), acc[r][1], 0, 0, 0);
                    }
                }
                float b8[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) b8[c] = a.bias ? a.bias[u * 32 + fc * 8 + c] : 0.f;
#pragma unroll
                for (int r = 0; r < UNR; ++r) {
                    bf16x8 o;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float x0 = acc[r][0][q] + b8[q], x1 = acc[r][1][q] + b8[4 + q];
                        o[q] = (xmc_h16)fmaxf(x0, x0 * one);
                        o[4 + q] = (xmc_h16)fmaxf(x1, x1 * one);
                    }
                    if (ok[r]) sc8[pix[r] * CO8 + u * 4 + fc] = o;
                }
            }
        }
    }
}

template <int KS, int TN, bool WLDS, bool POOL, int NW>      // KS = Cout / 32 K-steps of the data gradient, TN = Cin / 16 row blocks
__global__ __launch_bounds__(NW * 64, NW == 4 ? 2 : 1) void gentry_bwd_kernel(const GEntryArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char glds[];
    constexpr int C8 = TN * 2, CS8 = KS * 4, PPS = 64 / C8, NPAIR = C8 / 8;        // PPS pixels per wave step, NPAIR pairs of steps per group
    constexpr int RSTR = KS * 64 + 16, WBYTES = WLDS ? TN * 16 * RSTR : 0, SSTR = C8 * 16 + 16;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, fr = lane & 15, fc = lane >> 4;
    const int cc = lane % C8, pg = lane / C8;                    // the affine backward's roles: unit cc of pixel lane pg
    const u32x4* __restrict__ x16 = reinterpret_cast<const u32x4*>(a.x);
    const u32x4* __restrict__ dy16 = reinterpret_cast<const u32x4*>(a.dy);
    const u32x4* __restrict__ dsc16 = reinterpret_cast<const u32x4*>(a.dsc);
    unsigned char* const slab = glds + WBYTES + wv * 16 * SSTR;  // this wave's dskip: [16 slots][C8 units], rows padded by 16 bytes
    u32x4 wf[WLDS ? 1 : KS][WLDS ? 1 : TN];
    gentry_weights<KS, TN, WLDS, NW>(reinterpret_cast<const u32x4*>(a.wpk), glds, wf, tid, fr, fc);
    const float slope = a.slope;
    const int HW = a.H * a.W, Wq = a.W >> 1;
    const int nunits = POOL ? (a.H >> 1) * Wq : HW;              // quads or pixels of an image
    // slot f of group gl -> pixel of the image, or -1.  POOL: slot = (step s, pixel lane) with s & 1 the quad's row and the lane's low bit
    // its column; else 16 consecutive pixels
    auto slot_pixel = [&](int gl, int f) -> int {
        if constexpr (POOL) {
            const int s = f / PPS, pl = f % PPS;
            const int q = gl * 4 + (s >> 1) * (PPS / 2) + (pl >> 1);
            if (q >= nunits) return -1;
            const int qy = q / Wq, qx = q - qy * Wq;
            return (2 * qy + (s & 1)) * a.W + 2 * qx + (pl & 1);
        } else {
            const int p = gl * 16 + f;
            return p < nunits ? p : -1;
        }
    };
    float G0[8], B0[8], G1[8], B1[8], sg0[8], sb0[8], sg1[8], sb1[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) sg0[k] = sb0[k] = sg1[k] = sb1[k] = 0.f;
    // the sums of image n: over the pixel lanes of the wave, then one set of atomics (the accumulators arrive zero)
    auto flush = [&](int n) {
        float* const outs[4] = {a.dg0, a.db0, a.dg1, a.db1};
        float* const sums[4] = {sg0, sb0, sg1, sb1};
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                float v = sums[q][k];
#pragma unroll
                for (int o = C8; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
                if (lane < C8) atomicAdd(&outs[q][((size_t)n * C8 + cc) * 8 + k], v);
                sums[q][k] = 0.f;
            }
    };
    auto load_dsc = [&](int g, u32x4 (&pf)[KS]) {
        const int n = g / a.gpi, p = slot_pixel(g - n * a.gpi, fr);
        const size_t idx = ((size_t)n * HW + (p < 0 ? 0 : p)) * CS8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) pf[ks] = dsc16[idx + ks * 4 + fc];
    };
    // the affine backward's operands of step pair t of group g (a masked slot reads pixel 0 of the image and drops its results)
    struct PairOps { int px[2]; u32x4 xq[2], dq[2]; };
    auto load_pair = [&](int g, int t, PairOps& o) {
        const int n = g / a.gpi, gl = g - n * a.gpi;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            o.px[e] = slot_pixel(gl, (2 * t + e) * PPS + pg);
            const size_t idx = ((size_t)n * HW + (o.px[e] < 0 ? 0 : o.px[e])) * C8 + cc;
            o.xq[e] = x16[idx];
            o.dq[e] = dy16[idx];
        }
    };
    const int lo = blockIdx.x * a.per, hi = min(lo + a.per, a.nvg);
    int g = lo + wv, cur = -1;
    u32x4 pfs[KS];
    PairOps cu;
    constexpr bool PRE = KS < 4;          // the next group's dsc units in flight (KS = 4: their 16 registers are the ones that would spill)
    if (g < hi) { load_dsc(g, pfs); load_pair(g, 0, cu); }
    for (; g < hi; g += NW) {
        const int n = g / a.gpi, gl = g - n * a.gpi;
        if (n != cur) {
            if (cur >= 0) flush(cur);
            const size_t pb = ((size_t)n * C8 + cc) * 8;
#pragma unroll
            for (int k = 0; k < 8; ++k) { G0[k] = a.g0[pb + k]; B0[k] = a.b0[pb + k]; G1[k] = a.g1[pb + k]; B1[k] = a.b1[pb + k]; }
            cur = n;
        }
        u32x4 pfn[KS];
        if (PRE && g + NW < hi) load_dsc(g + NW, pfn);
        else {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) pfn[ks] = pfs[ks];
        }
        // dskip of the group's 16 slots: the 1x1 data gradient's MFMAs and epilogue (no bias, no activation: acc + 0 as there), rounded
#pragma unroll
        for (int u = 0; u < TN / 2; ++u) {
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                bf16x8 wa, wb;
                if constexpr (WLDS) {
                    const unsigned char* const wr = glds + (u * 32 + fr) * RSTR + fc * 16 + ks * 64;
                    wa = *reinterpret_cast<const bf16x8*>(wr);
                    wb = *reinterpret_cast<const bf16x8*>(wr + 16 * RSTR);
                } else {
                    wa = __builtin_bit_cast(bf16x8, wf[ks][2 * u]);
                    wb = __builtin_bit_cast(bf16x8, wf[ks][2 * u + 1]);
                }
                acc0 = XMC_MFMA_16x16x32(wa, __builtin_bit_cast(bf16x8, pfs[ks]), acc0, 0, 0, 0);
                acc1 = XMC_MFMA_16x16x32(wb, __builtin_bit_cast(bf16x8, pfs[ks]), acc1, 0, 0, 0);
            }
            bf16x8 o;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                o[q] = (xmc_h16)(acc0[q] + 0.f);
                o[4 + q] = (xmc_h16)(acc1[q] + 0.f);
            }
            *reinterpret_cast<bf16x8*>(slab + fr * SSTR + (u * 4 + fc) * 16) = o;
        }
        __builtin_amdgcn_wave_barrier();
        // the affine backward, one pair of steps at a time, the next pair's operands (or the next group's first) in flight
#pragma unroll 1
        for (int t = 0; t < NPAIR; ++t) {
            const bool more = t + 1 < NPAIR;
            const int gn = more ? g : g + NW;
            PairOps nx = cu;
            if (gn < hi) load_pair(gn, more ? t + 1 : 0, nx);
            float acc8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const bool live = cu.px[e] >= 0;
                const bf16x8 xb = __builtin_bit_cast(bf16x8, cu.xq[e]), db = __builtin_bit_cast(bf16x8, cu.dq[e]);
                const bf16x8 ob = *reinterpret_cast<const bf16x8*>(slab + ((2 * t + e) * PPS + pg) * SSTR + cc * 16);
                float xv[8], dv[8], ov[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) { xv[k] = (float)xb[k]; dv[k] = live ? (float)db[k] : 0.f; ov[k] = live ? (float)ob[k] : 0.f; }
                affine2_bwd_unit<XMC_BF16>(xv, dv, ov, true, true, slope, 1.f, nullptr, G0, B0, G1, B1, sg0, sb0, sg1, sb1);
                if (live) Vec8<XMC_BF16>::store(a.dx, ((size_t)n * HW + cu.px[e]) * C8 + cc, xv);
                if (POOL) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc8[k] += (float)(xmc_h16)xv[k];
                }
                __builtin_amdgcn_sched_barrier(0);          // one pixel after the other: interleaved, their temporaries do not fit
            }
            if (POOL) {
#pragma unroll
                for (int k = 0; k < 8; ++k) acc8[k] += __shfl_xor(acc8[k], C8, 64);       // the quad's other column: lane ^ C8
                const int q = gl * 4 + t * (PPS / 2) + (pg >> 1);
                if ((pg & 1) == 0 && cu.px[0] >= 0) Vec8<XMC_BF16>::store(a.dx_pool, ((size_t)n * nunits + q) * C8 + cc, acc8);
            }
            cu = nx;
        }
        __builtin_amdgcn_wave_barrier();          // the next group's dskip is written after these reads
        if (PRE) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) pfs[ks] = pfn[ks];
        } else if (g + NW < hi) {
            load_dsc(g + NW, pfs);
        }
    }
    if (cur >= 0) flush(cur);
}

// workgroups of `kernel` that are resident on the device at once
template <typename K>
int gentry_resident(K kernel, int threads, size_t lds) {
    int dev = 0, cus = 0, nb = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, threads, lds) != hipSuccess || nb < 1) nb = 1;
    (void)hipGetLastError();
    return cus * nb;
}

// grid (resident set, capped) and the groups per workgroup, a multiple of `unit`
inline int gentry_grid(GEntryArgs& a, int resident, int grid_cap, int unit) {
    int gx = resident;
    if (grid_cap > 0 && gx > grid_cap) gx = grid_cap;
    const int chunks = (a.nvg + unit - 1) / unit;
    if (gx > chunks) gx = chunks;
    a.per = (chunks + gx - 1) / gx * unit;
    return (a.nvg + a.per - 1) / a.per;
}

template <int KS, int TN, bool WLDS, int NW>
int launch_gentry_fwd(GEntryArgs& a, int grid_cap, hipStream_t st) {
    constexpr size_t lds = (WLDS ? TN * 16 * (KS * 64 + 16) : 0) + NW * 4 * KS * 32 * sizeof(float);
    auto kernel = gentry_fwd_kernel<KS, TN, WLDS, NW>;
    if (lds > 64 * 1024) XMC_ALLOW_BIG_LDS((*kernel));
    static const int resident = gentry_resident(kernel, NW * 64, lds);
    const int gx = gentry_grid(a, resident, grid_cap, 4);
    hipLaunchKernelGGL(kernel, dim3(gx), dim3(NW * 64), lds, st, a);
    xmc_note_kernel("gentry_fwd_kernel<%d, %d>", KS, TN);
    XMC_LAUNCH_CHECK();
    return 0;
}

template <int KS, int TN, bool WLDS, int NW>
int launch_gentry_bwd(GEntryArgs& a, int grid_cap, hipStream_t st) {
    constexpr size_t lds = (WLDS ? TN * 16 * (KS * 64 + 16) : 0) + NW * 16 * (TN * 2 * 16 + 16);
    if (a.dx_pool) {
        auto kernel = gentry_bwd_kernel<KS, TN, WLDS, true, NW>;
        if (lds > 64 * 1024) XMC_ALLOW_BIG_LDS((*kernel));
        static const int resident = gentry_resident(kernel, NW * 64, lds);
        hipLaunchKernelGGL(kernel, dim3(gentry_grid(a, resident, grid_cap, 1)), dim3(NW * 64), lds, st, a);
    } else {
        auto kernel = gentry_bwd_kernel<KS, TN, WLDS, false, NW>;
        if (lds > 64 * 1024) XMC_ALLOW_BIG_LDS((*kernel));
        static const int resident = gentry_resident(kernel, NW * 64, lds);
        hipLaunchKernelGGL(kernel, dim3(gentry_grid(a, resident, grid_cap, 1)), dim3(NW * 64), lds, st, a);
    }
    xmc_note_kernel("gentry_bwd_kernel<%d, %d, %d>", KS, TN, a.dx_pool ? 1 : 0);
    XMC_LAUNCH_CHECK();
    return 0;
}

// ---- 8 stored output channels (conv_out of the generator: 32 -> 3, df_gan.py:85-87, + bias + tanh).  On the 32-wide tile
// kernel this layer multiplies 32 output channels for the 8 it stores and is bound by that waste (0.66 ms where its 1.34 GB
// of tensors take 0.27 ms).  Here the output channels are the 16 rows of the MFMA (8 used), the B operand is the lane's
// 16-byte unit of the tap-shifted pixel read from a small LDS halo patch (pixel stride = channels + 16 bytes: conflict-free
// ds_read_b128), the weights (9 taps x Cin/32 fragments) stay in registers; 4 waves x 2 rows of an 8 x 16-pixel tile,
// 14-29 KB of LDS, persistent with the next patch prefetched into registers.
constexpr int TO_H = 8, TO_W = 16, TO_PH = TO_H + 2, TO_PW = TO_W + 2;
template <int KC>      // 32-channel K chunks per tap (Cin = 32 * KC)
__global__ __launch_bounds__(256, 2) void thin_out_kernel(const XmcConvDesc d, int tiles_x, int tiles_y, int ntiles) {
    constexpr int NKS = 9 * KC, CSU = 4 * KC, PSTR = CSU * 16 + 16;
    constexpr int NUN = TO_PH * TO_PW * CSU, MAXU = (NUN + 255) / 256;
    __shared__ __attribute__((aligned(16))) unsigned char smem[TO_PH * TO_PW * PSTR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, kb = lane >> 4;
    const u32x4* __restrict__ src = reinterpret_cast<const u32x4*>(d.src);
    const u32x4* __restrict__ wpk = reinterpret_cast<const u32x4*>(d.wpk);
    bf16x8 wa[NKS];
    int loff[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        loff[t] = ((d.dh[0][t] + 1) * TO_PW + d.dw[0][t] + 1 + col) * PSTR + kb * 16;
#pragma unroll
        for (int c = 0; c < KC; ++c)
            wa[t * KC + c] = __builtin_bit_cast(bf16x8, wpk[((size_t)d.wi[0][t] * d.CDw + col) * CSU + c * 4 + kb]);
    }
    float bias4[4] = {0.f, 0.f, 0.f, 0.f};
    if (d.bias && kb < 2) {
#pragma unroll
        for (int i = 0; i < 4; ++i) bias4[i] = d.bias[kb * 4 + i];
    }
    u32x4 pv[MAXU];
    auto prefetch = [&](int tile) {
        const int n = tile / (tiles_y * tiles_x), tr = tile - n * (tiles_y * tiles_x);
        const int y0 = (tr / tiles_x) * TO_H - 1, x0 = (tr % tiles_x) * TO_W - 1;
#pragma unroll
        for (int it = 0; it < MAXU; ++it) {
            const int id = tid + it * 256;
            const int pp = id / CSU, ch = id - pp * CSU;
            const int py = pp / TO_PW, px = pp - py * TO_PW;
            const int sy = y0 + py, sx = x0 + px;
            const bool ok = id < NUN && (unsigned)sy < (unsigned)d.SH && (unsigned)sx < (unsigned)d.SW;
            const u32x4 z = {0, 0, 0, 0};
            pv[it] = ok ? src[(((size_t)n * d.SH + sy) * d.SW + sx) * CSU + ch] : z;
        }
    };
    const XcdWalk xw = xmc_xcd_walk(ntiles);
    int tile = xw.first;
    if (tile < xw.end) prefetch(tile);
    for (; tile < xw.end; tile += xw.step) {
        __syncthreads();
#pragma unroll
        for (int it = 0; it < MAXU; ++it) {
            const int id = tid + it * 256;
            const int pp = id / CSU, ch = id - pp * CSU;
            if (id < NUN) *reinterpret_cast<u32x4*>(smem + pp * PSTR + ch * 16) = pv[it];
        }
        __syncthreads();
        if (tile + xw.step < xw.end) prefetch(tile + xw.step);
        const int n = tile / (tiles_y * tiles_x), tr = tile - n * (tiles_y * tiles_x);
        const int y0 = (tr / tiles_x) * TO_H, x0 = (tr % tiles_x) * TO_W;
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const int r = wave * 2 + rr;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int c = 0; c < KC; ++c) {
                    const bf16x8 b = *reinterpret_cast<const bf16x8*>(smem + r * TO_PW * PSTR + loff[t] + c * 64);
                    acc = XMC_MFMA_16x16x32(wa[t * KC + c], b, acc, 0, 0, 0);
                }
            if (kb < 2) {                                  // D[row = output channel kb*4 + i][col = pixel]; 8 channels stored
                bf16x4 o;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float v = acc[i] + bias4[i];
                    if (d.act == XMC_ACT_TANH) v = tanh_fast(v);
                    else if (d.act == XMC_ACT_LRELU) v = lrelu_f(v);
                    o[i] = (xmc_h16)v;
                }
                const size_t p = ((size_t)n * d.DH + y0 + r) * d.DW + x0 + col;
                *reinterpret_cast<bf16x4*>(reinterpret_cast<xmc_h16*>(d.dst) + p * 8 + kb * 4) = o;
            }
        }
    }
}

}  // namespace

// 0 = launched, 1 = not this kernel's case, < 0 = error
int xmc_conv_thin_out_try(const XmcConvDesc* d, void* stream) {
    static const bool off = xmc_debug_off("no_thin_out");
    if (off) return 1;
    if (d->dtype != XMC_BF16 || d->out_dtype != XMC_BF16 || d->CD != 8 || (d->CS != 32 && d->CS != 64) || d->CDw < 16) return 1;
    if (d->SA != 1 || d->DA != 1 || d->src_shift != 0 || d->nclass != 1 || d->ntaps != 9 || d->groups > 1) return 1;
    if (d->res || d->mask || d->alpha_dev || d->dst2 || d->dst_pool || d->post_act || d->sign_bits || d->dot) return 1;
    if (d->act != XMC_ACT_NONE && d->act != XMC_ACT_TANH && d->act != XMC_ACT_LRELU) return 1;
    if (d->MH % TO_H != 0 || d->MW % TO_W != 0 || !xmc_same_size_maps(d)) return 1;
    if (d->dph[0] != 0 || d->dpw[0] != 0 || !xmc_taps_within(d, 0, 1)) return 1;
    const int tx = d->MW / TO_W, ty = d->MH / TO_H, ntiles = d->N * tx * ty;
    const int grid = ntiles < 256 * 8 ? ntiles : 256 * 8;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const XmcKName name = {"thin_out_kernel<%d>", {d->CS / 32}};
    if (d->CS == 32) return xmc_launch<&thin_out_kernel<1>, false>(dim3(xmc_ab_grid(grid)), dim3(256), 0, st, name, *d, tx, ty, ntiles);
    return xmc_launch<&thin_out_kernel<2>, false>(dim3(xmc_ab_grid(grid)), dim3(256), 0, st, name, *d, tx, ty, ntiles);
}

// 0 = launched, 1 = not this kernel's case, < 0 = error
int xmc_conv_thin_try(const XmcConvDesc* d, void* stream) {
    static const bool off = xmc_debug_off("no_thin");
    if (off) return 1;
    if (d->dtype != XMC_BF16 || d->out_dtype != XMC_BF16 || d->CS != 8) return 1;
    if (d->SA != 1 || d->DA != 1 || d->src_shift != 0 || d->nclass != 1 || d->ntaps > 12) return 1;
    if (d->CDw != 32 && d->CDw != 64) return 1;
    if (d->res || d->alpha_dev || d->dst2 || d->post_act || d->sign_bits || d->dot || (d->act != XMC_ACT_NONE && d->act != XMC_ACT_LRELU)) return 1;
    if (d->MH % 8 != 0 || d->MW % 32 != 0 || !xmc_same_size_maps(d)) return 1;
    if (d->dph[0] != 0 || d->dpw[0] != 0) return 1;
    const XmcTapBox b = xmc_tap_box(d, 0);
    if (b.hmax - b.hmin > 4 || b.wmax - b.wmin > 4 || b.hmin > 0 || b.wmin > 0 || b.hmax < 0 || b.wmax < 0) return 1;
    ThinCfg t;
    t.tiles_y = d->MH / 8; t.tiles_x = d->MW / 32;
    t.PH = 8 + (b.hmax - b.hmin); t.PW = 32 + (b.wmax - b.wmin);
    t.dh0 = b.hmin; t.dw0 = b.wmin;
    if (t.PH * t.PW > 512) return 1;
    const int ntiles = d->N * t.tiles_y * t.tiles_x;
    int gx = 256 * 5;
    if (gx > ntiles) gx = ntiles;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const XmcKName name = {"thin_in_kernel<%d>", {d->CDw}};
    if (d->CDw == 32) return xmc_launch<&thin_in_kernel<32>, false>(dim3(xmc_ab_grid(gx)), dim3(256), 0, st, name, *d, t, ntiles);
    return xmc_launch<&thin_in_kernel<64>, false>(dim3(xmc_ab_grid(gx)), dim3(256), 0, st, name, *d, t, ntiles);
}

// The generator tail's backward in one pass (gtail_bwd_kernel; include/xmc_gan_hip.h).  0 = launched, 1 = not this kernel's case, < 0 = error
extern "C" int xmc_gtail_bwd(const XmcConvDesc* d, const void* img, float* dwp, float* dbias, int dw_rows, int grid_cap, void* stream) {
    if (!d || !d->src || !d->wpk || !d->dst || !d->mask || !img) return XMC_EINVAL;
    if (d->N < 1 || d->MH < 1 || d->MW < 1 || d->ntaps < 1 || d->ntaps > XMC_MAX_TAPS) return XMC_ESHAPE;
    if (dwp && (dw_rows < 4 || dw_rows % 4 != 0)) return XMC_ESHAPE;
    if (d->mask_bits || d->sc_img || d->wpk_lo) return XMC_EINVAL;
    static const bool off = xmc_debug_off("no_gtail_fused");
    if (off) return 1;
    if (d->dtype != XMC_BF16 || d->out_dtype != XMC_BF16 || d->CS != 8 || d->CD != 32 || d->CDw != 32) return 1;
    if (d->SA != 1 || d->DA != 1 || d->src_shift != 0 || d->nclass != 1 || d->ntaps != 9 || d->groups > 1) return 1;
    if (d->bias || d->res || d->alpha_dev || d->dst2 || d->post_act || d->sign_bits || d->dot || d->act != XMC_ACT_NONE) return 1;
    if (d->MH % 8 != 0 || d->MW % 2 != 0 || !xmc_same_size_maps(d)) return 1;
    if (d->dph[0] != 0 || d->dpw[0] != 0) return 1;
    for (int t = 0; t < 9; ++t)         // the 3x3, pad-1 data gradient in its natural tap order: tap t reads dpre at (+1 - t / 3, +1 - t % 3)
        if (d->dh[0][t] != 1 - t / 3 || d->dw[0][t] != 1 - t % 3 || d->wi[0][t] != t) return 1;
    const int tiles_y = d->MH / 8, tiles_x = (d->MW + 31) / 32;
    if ((int64_t)d->N * d->MH * d->MW * 4 >= (1ll << 31) || (int64_t)d->N * tiles_y * tiles_x >= (1ll << 30)) return 1;
    const int ntiles = d->N * tiles_y * tiles_x;
    int gx = 256 * (dwp ? 3 : 5);       // the resident set (see the kernel's register note); without the weight gradient as thin_in_kernel
    if (grid_cap > 0 && gx > grid_cap) gx = grid_cap;
    if (gx > ntiles) gx = ntiles;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const u32x4* img16 = reinterpret_cast<const u32x4*>(img);
    if (dwp) hipLaunchKernelGGL((gtail_bwd_kernel<true>), dim3(xmc_ab_grid(gx)), dim3(256), 0, st, *d, img16, dwp, dbias, dw_rows, tiles_y, tiles_x, ntiles);
    else hipLaunchKernelGGL((gtail_bwd_kernel<false>), dim3(xmc_ab_grid(gx)), dim3(256), 0, st, *d, img16, nullptr, nullptr, 0, tiles_y, tiles_x, ntiles);
    xmc_note_kernel("gtail_bwd_kernel<%d>", dwp ? 1 : 0);
    XMC_LAUNCH_CHECK();
    return 0;
}

// The entry of a generator block with a learned shortcut, one pass per direction (gentry_fwd_kernel / gentry_bwd_kernel;
// include/xmc_gan_hip.h).  0 = launched, 1 = not these kernels' case, < 0 = error
static int gentry_case(int N, int H, int W, int Cin, int Cout, int dtype) {
    static const bool off = xmc_debug_off("no_gentry_fused");
    if (off || dtype != XMC_BF16) return 1;
    if (!((Cin == 64 && Cout == 32) || (Cin == 128 && Cout == 64) || (Cin == 256 && Cout == 128))) return 1;
    if ((int64_t)N * H * W * (Cin / 8) >= (1ll << 31) || (int64_t)N * ((int64_t)H * W / 16 + 4) >= (1ll << 30)) return 1;
    return 0;
}

extern "C" int xmc_gentry_fwd(const void* x, const float* g0, const float* b0, const float* g1, const float* b1, const void* wpk, const float* bias,
                              void* h, void* sc, int N, int H, int W, int Cin, int Cout, int wrows, float slope, int dtype, int grid_cap, void* stream) {
    if (!x || !g0 || !b0 || !g1 || !b1 || !wpk || !h || !sc) return XMC_EINVAL;
    if (N < 1 || H < 1 || W < 1 || Cin < 8 || Cout < 8 || Cin % 8 || Cout % 8) return XMC_ESHAPE;
    if (const int rc = gentry_case(N, H, W, Cin, Cout, dtype)) return rc;
    if (wrows != Cout) return 1;                           // the packed weights [Cout][Cin], rows unpadded
    GEntryArgs a = {};
    a.x = x; a.wpk = wpk; a.h = h; a.sc = sc; a.bias = bias;
    a.g0 = g0; a.b0 = b0; a.g1 = g1; a.b1 = b1;
    a.N = N; a.H = H; a.W = W; a.slope = slope;
    a.gpi = ((H * W + 15) / 16 + 3) / 4 * 4;               // 16-pixel groups of an image, padded to the four a wave has in flight
    a.nvg = N * a.gpi;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (Cin == 64) return launch_gentry_fwd<2, 2, false, 4>(a, grid_cap, st);
    if (Cin == 128) return launch_gentry_fwd<4, 4, true, 4>(a, grid_cap, st);
    return launch_gentry_fwd<8, 8, true, 8>(a, grid_cap, st);
}

extern "C" int xmc_gentry_bwd(const void* x, const void* dy, const void* dsc, const float* g0, const float* b0, const float* g1, const float* b1,
                              const void* wpk_t, void* dx, void* dx_pool, float* dg0, float* db0, float* dg1, float* db1, int N, int H, int W,
                              int Cin, int Cout, int wrows, float slope, int dtype, int grid_cap, void* stream) {
    if (!x || !dy || !dsc || !g0 || !b0 || !g1 || !b1 || !wpk_t || !dx || !dg0 || !db0 || !dg1 || !db1) return XMC_EINVAL;
    if (N < 1 || H < 1 || W < 1 || Cin < 8 || Cout < 8 || Cin % 8 || Cout % 8) return XMC_ESHAPE;
    if (const int rc = gentry_case(N, H, W, Cin, Cout, dtype)) return rc;
    if (wrows != Cin) return 1;
    if (dx_pool && ((H & 1) || (W & 1))) return 1;
    GEntryArgs a = {};
    a.x = x; a.dy = dy; a.dsc = dsc; a.wpk = wpk_t; a.dx = dx; a.dx_pool = dx_pool;
    a.g0 = g0; a.b0 = b0; a.g1 = g1; a.b1 = b1;
    a.dg0 = dg0; a.db0 = db0; a.dg1 = dg1; a.db1 = db1;
    a.N = N; a.H = H; a.W = W; a.slope = slope;
    a.gpi = dx_pool ? ((H / 2) * (W / 2) + 3) / 4 : (H * W + 15) / 16;         // groups of four 2x2 quads, or of 16 pixels
    a.nvg = N * a.gpi;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (Cin == 64) return launch_gentry_bwd<1, 4, false, 4>(a, grid_cap, st);
    if (Cin == 128) return launch_gentry_bwd<2, 8, true, 4>(a, grid_cap, st);
    return launch_gentry_bwd<4, 16, true, 8>(a, grid_cap, st);
}

// 0 = launched, 1 = not this kernel's case, < 0 = error
static int pw1x1_go(const XmcConvDesc* d, void* stream, const unsigned char* sbits, void* smasked, float mslope) {
    static const bool off = xmc_debug_off("no_pw1x1");
    if (off) return 1;
    if (d->dtype != XMC_BF16 || d->out_dtype != XMC_BF16) return 1;
    if (d->ntaps != 1 || d->nclass != 1 || d->SA != 1 || d->DA != 1 || d->src_shift != 0) return 1;
    if (d->dh[0][0] != 0 || d->dw[0][0] != 0 || d->dph[0] != 0 || d->dpw[0] != 0) return 1;
    if (!xmc_same_size_maps(d)) return 1;
    if (d->post_act || d->sign_bits || d->dot) return 1;
    if (d->res || d->mask || d->alpha_dev || d->dst2 || (d->act != XMC_ACT_NONE && d->act != XMC_ACT_LRELU)) return 1;
    if (d->CS % 32 != 0 || d->CDw % 32 != 0 || d->CD % 8 != 0) return 1;
    const int64_t M = (int64_t)d->N * d->MH * d->MW;
    if (M % 16 != 0 || M / 16 >= (1ll << 31) || M < 16 * 1024) return 1;
    const int ngroups = (int)(M / 16);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int ks = d->CS / 32, tn = d->CDw / 16;
    // more weight fragments than a wave's registers hold: weights in LDS (Cin 128 or 256, any Cout)
    static const bool no_w = xmc_debug_off("no_pw1x1_lds");
    if (!no_w && (ks == 4 || ks == 8) && ks * tn > 16 && d->CDw >= 128 && M >= 32 * 1024)
        return ks == 4 ? launch_pww<4>(*d, ngroups, st, sbits, smasked, mslope) : launch_pww<8>(*d, ngroups, st, sbits, smasked, mslope);
    if (d->CS > 128 || d->CDw > 128) return 1;
    if (ks * tn > 16 || ks == 3) return 1;
#define PW_CASE(K, T) if (ks == K && tn == T) return launch_pw<K, T>(*d, ngroups, st, sbits, smasked, mslope);
    PW_CASE(1, 2) PW_CASE(1, 4) PW_CASE(1, 8) PW_CASE(2, 2) PW_CASE(2, 4) PW_CASE(2, 8) PW_CASE(4, 2) PW_CASE(4, 4)
#undef PW_CASE
    return 1;
}

int xmc_conv_pw1x1_try(const XmcConvDesc* d, void* stream) { return d->wpk_lo ? 1 : pw1x1_go(d, stream, nullptr, nullptr, 0.f); }

// The same kernels on a weight PAIR (XmcConvDesc.wpk_lo, ABI 12): two MFMAs per K step.  1 = not one of their shapes.
extern "C" int xmc_conv_pw1x1_split(const XmcConvDesc* d, void* stream) {
    if (!d || !d->src || !d->wpk || !d->wpk_lo || !d->dst) return XMC_EINVAL;
    if (d->ntaps != 1 || d->CS % 8 != 0 || d->CD % 8 != 0 || d->CDw % 32 != 0 || d->CDw < d->CD || d->N < 1 || d->MH < 1 || d->MW < 1) return XMC_ESHAPE;
    if (d->mask_bits || d->sc_img) return XMC_EINVAL;
    static const bool off = xmc_debug_off("no_pw1x1_split");
    if (off) return 1;
    return pw1x1_go(d, stream, nullptr, nullptr, 0.f);
}

// The 1x1 convolution of `d` on the streaming kernels only, with the masked copy of its SOURCE as a by-product (see mask_unit):
// src_masked[unit] = src[unit] x LeakyReLU'(bit) from one sign byte per 8-channel unit (XmcConvDesc.sign_bits layout of the source
// tensor).  Returns 1 and launches nothing when the shape is not one of theirs -- the caller then runs xmc_conv_igemm and
// xmc_signmask_apply separately.
extern "C" int xmc_conv_pw1x1_masked_src(const XmcConvDesc* d, const void* src_bits, void* src_masked, float slope, void* stream) {
    if (!d || !d->src || !d->wpk || !d->dst || !src_bits || !src_masked) return XMC_EINVAL;
    if (d->ntaps != 1 || d->CS % 8 != 0 || d->CD % 8 != 0 || d->CDw % 32 != 0 || d->CDw < d->CD || d->N < 1 || d->MH < 1 || d->MW < 1) return XMC_ESHAPE;
    static const bool off = xmc_debug_off("no_pw1x1_masked_src");
    if (off) return 1;
    return pw1x1_go(d, stream, static_cast<const unsigned char*>(src_bits), src_masked, slope);
}
