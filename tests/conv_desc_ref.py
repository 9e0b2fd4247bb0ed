"""An f64 numpy interpreter of XmcConvDesc's index space (include/xmc_gan_hip.h, the paragraph above the struct); a helper, not a test.
It reads the fields of the ctypes structure and nothing else of the product, so a descriptor the product builds can be executed, and
held against torch, without a GPU.

For class z, row m -> (n, a, b) with a < MH, b < MW, and tap t:
  source pixel       (a*SA + dh[z][t], b*SA + dw[z][t]), zero outside [0, SH << src_shift) x [0, SW << src_shift), then >> src_shift;
  destination pixel  (a*DA + dph[z], b*DA + dpw[z]);
  weight slice       slices[wi[z][t]] : [CD][CS].
No epilogue is modelled (bias, activation, alpha, mask, residual, the second outputs), nor `groups`: the slices are dense."""
import numpy as np


def run(d, src, slices):
    """src f64 [N, SH, SW, CS], slices f64 [nslices, CD, CS] -> (dst f64 [N, DH, DW, CD], how often each dst pixel was written [DH, DW])"""
    assert src.shape == (d.N, d.SH, d.SW, d.CS) and slices.shape[1:] == (d.CD, d.CS), (src.shape, slices.shape)
    sh = d.src_shift
    VH, VW = d.SH << sh, d.SW << sh
    a, b = np.arange(d.MH), np.arange(d.MW)
    dst = np.zeros((d.N, d.DH, d.DW, d.CD))
    writes = np.zeros((d.DH, d.DW), dtype=np.int64)
    for z in range(d.nclass):
        acc = np.zeros((d.N, d.MH, d.MW, d.CD))
        for t in range(d.ntaps):
            sy, sx = a * d.SA + d.dh[z][t], b * d.SA + d.dw[z][t]
            inside = ((sy >= 0) & (sy < VH))[:, None] & ((sx >= 0) & (sx < VW))[None, :]
            rows, cols = np.clip(sy, 0, VH - 1) >> sh, np.clip(sx, 0, VW - 1) >> sh
            patch = src[:, rows[:, None], cols[None, :], :] * inside[None, :, :, None]          # [N, MH, MW, CS]
            acc += patch @ slices[d.wi[z][t]].T
        dy, dx = a * d.DA + d.dph[z], b * d.DA + d.dpw[z]
        assert dy.min() >= 0 and dy.max() < d.DH and dx.min() >= 0 and dx.max() < d.DW, (z, dy, dx)
        dst[:, dy[:, None], dx[None, :], :] = acc
        np.add.at(writes, (dy[:, None], dx[None, :]), 1)
    return dst, writes


# csrc/pointwise.hip, above the pack kernels: output parity i of the fused nearest x2 upsample + 3x3 convolution sees two low-resolution
# rows, each the sum of the kernel rows that land on it -- i=0: {0} | {1,2}, i=1: {0,1} | {2}; the same for columns.
_UP_ROWS = (((0,), (1, 2)), ((0, 1), (2,)))


def upconv_slices(w):
    """w f64 [Co, Ci, 3, 3] -> the 16 pre-summed slices [16, Co, Ci], slice (i*2 + j)*4 + th*2 + tw"""
    out = np.zeros((16,) + w.shape[:2])
    for i in range(2):
        for j in range(2):
            for th in range(2):
                for tw in range(2):
                    out[(i * 2 + j) * 4 + th * 2 + tw] = sum(w[:, :, kh, kw] for kh in _UP_ROWS[i][th] for kw in _UP_ROWS[j][tw])
    return out
