"""Plain-torch restatement of the differentiable augmentation (xmc_gan_hip.h: xmc_diffaug_apply), in f64 unless the inputs say otherwise.

Images are [N,C,H,W] here (the real channels only); a parameter row is (b, s, c, tx, ty, cy, cx, 0).  `forward` is the affine map
y = A x + (b-term), `linear` is A x, `transpose` is A^T g, each written from the definition and independently of the other two."""
import torch


def _geometry(P, H, W, cut):
    """mask [N,H,W] of output pixels that take a source value, and the source coordinates (clamped where the mask is off)"""
    N = P.shape[0]
    ii = torch.arange(H).view(1, H, 1).expand(N, H, W)
    jj = torch.arange(W).view(1, 1, W).expand(N, H, W)
    tx, ty, cy, cx = (P[:, k].round().long().view(N, 1, 1) for k in (3, 4, 5, 6))
    si, sj = ii + ty, jj + tx
    inside = (si >= 0) & (si < H) & (sj >= 0) & (sj < W)
    cutm = (ii >= cy) & (ii < cy + cut) & (jj >= cx) & (jj < cx + cut)
    return inside & ~cutm, si.clamp(0, H - 1), sj.clamp(0, W - 1)


def _colour(x, P, with_b):
    N = x.shape[0]
    b, s, c = (P[:, k].to(x.dtype).view(N, 1, 1, 1) for k in (0, 1, 2))
    u = x + b if with_b else x
    p = u.mean(dim=1, keepdim=True)
    v = s * u + (1 - s) * p
    m = v.mean(dim=(1, 2, 3), keepdim=True)
    return c * v + (1 - c) * m


def _place(w, P, cut):
    N, C, H, W = w.shape
    keep, si, sj = _geometry(P, H, W, cut)
    n = torch.arange(N).view(N, 1, 1).expand(N, H, W)
    g = w.permute(0, 2, 3, 1)[n, si, sj]                  # [N,H,W,C]: w at the source of every output pixel
    return (g * keep.unsqueeze(-1).to(w.dtype)).permute(0, 3, 1, 2)


def forward(x, P, cut):
    """colour, then translation with zero fill, then cutout"""
    return _place(_colour(x, P, True), P, cut)


def linear(x, P, cut):
    """the linear part A x (b ignored)"""
    return _place(_colour(x, P, False), P, cut)


def transpose(dy, P, cut):
    """A^T dy by the formulas of the backward pass: scatter dy back to its sources, then the transposes of contrast and saturation"""
    N, C, H, W = dy.shape
    keep, si, sj = _geometry(P, H, W, cut)
    g = torch.zeros_like(dy)
    for n in range(N):                                    # (an output pixel has one source: no collisions)
        k = keep[n]
        g[n][:, si[n][k], sj[n][k]] = dy[n][:, k]
    s, c = (P[:, k].to(dy.dtype).view(N, 1, 1, 1) for k in (1, 2))
    G = g.sum(dim=(1, 2, 3), keepdim=True)
    dv = c * g + (1 - c) * G / (C * H * W)
    return s * dv + (1 - s) * dv.mean(dim=1, keepdim=True)


def amplification(P, xmax):
    """A of the error bound, per image: (max|x| + |b|)(|s| + |1-s|)(|c| + |1-c|)"""
    b, s, c = (P[:, k].double() for k in (0, 1, 2))
    return (xmax + b.abs()) * (s.abs() + (1 - s).abs()) * (c.abs() + (1 - c).abs())


def bound(ref, P, xmax, u16, n_img):
    """per element: u16 |ref| + 2^-24 (16 + n_img) A  (u16: unit roundoff of the output format; n_img = C*H*W: any-order f32 sum)"""
    A = amplification(P, xmax).view(-1, 1, 1, 1)
    return u16 * ref.abs().double() + 2.0 ** -24 * (16 + n_img) * A
