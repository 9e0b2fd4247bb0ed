// Host-side plans of the halo-tile convolutions (conv_tile.hip, conv_wtile.hip, conv_wtile3.hip, conv_thin.hip): integer arithmetic on
// XmcConvDesc and nothing else -- no HIP type, no XMC_DEBUG_DISPATCH read -- so that it compiles with a plain C++ compiler and is tested
// without a GPU (tests/test_conv_plan_cpu.py).  A switch a plan depends on is read in the .hip file and arrives here as an argument.
#pragma once
#include <stdint.h>

#include "xmc_gan_hip.h"

// bounding box of the tap offsets (dh, dw) of class z
struct XmcTapBox { int hmin, hmax, wmin, wmax; };
static inline XmcTapBox xmc_tap_box(const XmcConvDesc* d, int z) {
    XmcTapBox b = {127, -128, 127, -128};
    for (int k = 0; k < d->ntaps; ++k) {
        const int h = d->dh[z][k], w = d->dw[z][k];
        b.hmin = h < b.hmin ? h : b.hmin; b.hmax = h > b.hmax ? h : b.hmax;
        b.wmin = w < b.wmin ? w : b.wmin; b.wmax = w > b.wmax ? w : b.wmax;
    }
    return b;
}
// every tap of class z within +-r of the centre
static inline bool xmc_taps_within(const XmcConvDesc* d, int z, int r) {
    const XmcTapBox b = xmc_tap_box(d, z);
    return b.hmin >= -r && b.hmax <= r && b.wmin >= -r && b.wmax <= r;
}
// source, GEMM grid and destination are maps of one size (unit strides, no upsample)
static inline bool xmc_same_size_maps(const XmcConvDesc* d) { return d->SH == d->MH && d->SW == d->MW && d->DH == d->MH && d->DW == d->MW; }

// The plan of the streamed-weights kernels: a kernel argument of wtile2_kernel as it stands, of wtile3_kernel with `ipt` behind it.
struct XmcHaloPlan {
    int TH, TW, log2TW;                                  // output tile (TH * TW == 256)
    int tiles_y, tiles_x;                                // tiles per image
    int PH[XMC_MAX_CLASSES], PW[XMC_MAX_CLASSES];        // patch size per class
    int dh0[XMC_MAX_CLASSES], dw0[XMC_MAX_CLASSES];      // min tap offsets per class (mode 0)
    int nslab;                                           // K slabs per tile: CS/64 (mode 0), 4*CS/64 (mode 1)
    int patch_bytes;                                     // one patch buffer, set by the kernel's own plan
    int8_t tsel[4][4];                                   // mode 1: tap index of (dy*2+dx, ta*2+tb)
};
static_assert(sizeof(XmcHaloPlan) == 108 && __builtin_offsetof(XmcHaloPlan, nslab) == 84 && __builtin_offsetof(XmcHaloPlan, tsel) == 92,
              "XmcHaloPlan is a kernel argument: its layout is what the kernels were built against");

// What the streamed-weights plans have in common: every check and every member but patch_bytes.  Returns 1 when the descriptor is a
// case of these kernels.  *mode 0: unit source stride, 3x3 or 2x2 tap sets; 1: the 16 taps of a 4x4 stride-2 layer.
// ipt: images per tile -- 1, or 4 where the caller has found an 8 x 8 map whose tile is four whole images side by side (8 x 32, one tile
// per image group; the caller lays out the patch columns itself).
static inline int xmc_halo_plan(const XmcConvDesc* d, XmcHaloPlan* t, int* mode, int ipt) {
    if (d->dtype != XMC_BF16 || d->out_dtype != XMC_BF16 || d->src_shift != 0) return 0;
    if (d->CS % 64 != 0 || d->CS > 64 * 64 / 4) return 0;
    const bool mi = ipt > 1;
    if (!mi && d->MW % 16 != 0) return 0;
    const int TW = (mi || d->MW >= 32) ? 32 : 16, TH = 256 / TW;
    if (!mi && (d->MH % TH != 0 || d->MW % TW != 0)) return 0;
    t->TH = TH; t->TW = TW; t->log2TW = TW == 32 ? 5 : 4;
    t->tiles_y = mi ? 1 : d->MH / TH; t->tiles_x = mi ? 1 : d->MW / TW;
    if (d->SA == 1) {
        if (d->ntaps != 9 && d->ntaps != 4) return 0;
        if (d->SH != d->MH || d->SW != d->MW) return 0;
        *mode = 0;
        t->nslab = d->CS / 64;
        for (int z = 0; z < d->nclass; ++z) {
            const XmcTapBox b = xmc_tap_box(d, z);
            // halo depth <= tile size (a halo row is outside the image only for tiles on that border)
            if (b.hmin < -TH || b.hmax > TH || b.wmin < -TW || b.wmax > TW) return 0;
            t->dh0[z] = b.hmin; t->dw0[z] = b.wmin;
            t->PH[z] = TH + (b.hmax - b.hmin); t->PW[z] = TW + (b.wmax - b.wmin);
        }
    } else if (d->SA == 2) {
        if (d->ntaps != 16 || d->nclass != 1 || d->DA != 1 || d->SH != 2 * d->MH || d->SW != 2 * d->MW) return 0;
        *mode = 1;
        t->nslab = 4 * (d->CS / 64);
        if (t->nslab > 64) return 0;
        // slab group g = (dy, dx) of the space-to-depth view, tap tp = (ta, tb) of its dense 2x2: the one tap of the 4x4 at that offset
        for (int g = 0; g < 4; ++g)
            for (int tp = 0; tp < 4; ++tp) {
                const int wh = 2 * (tp >> 1) + (g >> 1) - 1, ww = 2 * (tp & 1) + (g & 1) - 1;
                int found = -1;
                for (int k = 0; k < 16; ++k)
                    if (d->dh[0][k] == wh && d->dw[0][k] == ww) found = found < 0 ? k : 99;
                if (found < 0 || found > 15) return 0;         // missing or duplicated
                t->tsel[g][tp] = (int8_t)found;
            }
        t->PH[0] = TH + 1; t->PW[0] = TW + 1; t->dh0[0] = t->dw0[0] = 0;
    } else {
        return 0;
    }
    if (d->dst_pool && (d->DA != 1 || d->nclass != 1 || (d->DH & 1) || (d->DW & 1))) return 0;
    if (d->res_mode == 2 && d->DA != 1) return 0;
    // 32-bit unit offsets in the kernels
    if ((int64_t)d->N * d->SH * d->SW * (d->CS / 8) >= (1ll << 31) || (int64_t)d->N * d->DH * d->DW * (d->CD / 8) >= (1ll << 31)) return 0;
    return 1;
}
// pixels of the largest patch over the classes of a plan
static inline int xmc_halo_max_patch(const XmcConvDesc* d, const XmcHaloPlan* t) {
    int m = 0;
    for (int z = 0; z < d->nclass; ++z) m = t->PH[z] * t->PW[z] > m ? t->PH[z] * t->PW[z] : m;
    return m;
}
