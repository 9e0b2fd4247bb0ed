"""Sampling from a trained generator: latent draws, the forward in evaluation mode, images as uint8 on the device, reranking by the
discriminator's conditional logit.  `xmc_gan/sample.py` is the command line over this module.

The image leaves the device as uint8 [n,S,S,3] (`ops.image_to_u8`, csrc/image.hip): a quarter of the bytes of the f32 NCHW batch the
trainer's `eval()` copies, and already what a PNG encoder wants.  Nothing here trains: every forward runs under ``torch.no_grad()`` with
the network in evaluation mode, and its ``training`` flag is put back afterwards.

Every forward also runs inside ``ops.fixed_order()``: the GroupNorm statistics and the word-region pooling of the attention generators are
f32 sums that the training step accumulates with atomics from many workgroups, so two forwards of the same inputs differ in their last
bits there -- enough to move a uint8 pixel.  With one workgroup per reduction target the same noise and captions give the same bytes,
for every generator; the cost is the parallelism of those few small launches, which sampling does not miss.
"""
import inspect

import torch

from . import ops


def truncated_noise(n, dim, seed, psi=None):
    """f32 [n, dim] on the CPU from ``torch.Generator().manual_seed(seed)`` (the trainer draws its noise on the CPU too).
    ``psi=None``: exactly ``torch.randn(n, dim, generator=g)``.  Otherwise the truncation trick by resampling: the entries with
    |z| > psi are drawn again from the same generator, all of them in one call in row-major order, until none is left; an entry that
    was inside on the first draw keeps its value."""
    g = torch.Generator().manual_seed(int(seed))
    z = torch.randn(int(n), int(dim), generator=g)
    if psi is None:
        return z
    psi = float(psi)
    if not psi > 0.0:
        raise ValueError(f"truncation psi must be > 0, got {psi}")
    while True:
        out = z.abs() > psi
        k = int(out.sum())
        if k == 0:
            return z
        z[out] = torch.randn(k, generator=g)


def slerp(a, b, t):
    """row-wise spherical interpolation of a, b [n, d] at t (a number, or [n] / [n, 1]): sin((1-t) w) / sin(w) a + sin(t w) / sin(w) b
    with w the angle between the rows.  Exact at t = 0 and t = 1; rows whose angle has a sine below 1e-6 (parallel, opposite or zero)
    are interpolated linearly, so a == b gives a and never NaN."""
    a, b = torch.as_tensor(a).float(), torch.as_tensor(b).float()
    t = torch.as_tensor(t, dtype=torch.float32, device=a.device)
    if t.dim() < 2:
        t = t.reshape(-1, 1)
    an = a / a.norm(dim=-1, keepdim=True).clamp_min(1e-30)
    bn = b / b.norm(dim=-1, keepdim=True).clamp_min(1e-30)
    w = torch.acos((an * bn).sum(-1, keepdim=True).clamp(-1.0, 1.0))
    so = torch.sin(w)
    lin = (1.0 - t) * a + t * b
    sph = torch.sin((1.0 - t) * w) / so * a + torch.sin(t * w) / so * b
    return torch.where(so < 1e-6, lin, sph)


class _eval_mode:
    """modules in evaluation mode, their ``training`` flags restored on the way out"""

    def __init__(self, *modules):
        self.modules = [m for m in modules if m is not None]

    def __enter__(self):
        self.was = [m.training for m in self.modules]
        for m in self.modules:
            m.eval()

    def __exit__(self, *a):
        for m, w in zip(self.modules, self.was):
            m.train(w)
        return False


def _rows(t, i, j):
    return None if t is None else t[i:j]


class Sampler:
    """``Sampler(netG, netD=None)``: images, discriminator scores and best-of-m reranking from the two networks as they are (weights are
    read, never written).  ``separate``: whether the discriminator takes the raw sentence embedding (cfg.DISC.SEPERATE) instead of the
    generator's projection of it; None reads the live cfg."""

    def __init__(self, netG, netD=None, separate=None):
        self.netG, self.netD = netG, netD
        self.device = next(netG.parameters()).device
        if separate is None:
            from xmc_gan.config.gan import cfg
            separate = bool(cfg.DISC.SEPERATE)
        self.separate = bool(separate)
        # the discriminator's engine-layout entrance (model/df_gan.py NetD.forward(x, nhwc8=)); one without it gets the NCHW image
        self._d_nhwc = netD is not None and "nhwc8" in inspect.signature(netD.forward).parameters

    def engine_images(self, noise, sent_embs, words_embs=None, mask=None):
        """one forward: the image in the engine layout [n,S,S,8] (activation dtype, channels 0..2).  Call it under `_eval_mode`."""
        netG = self.netG
        kw = dict(noise=noise.to(self.device), sent_embs=sent_embs, words_embs=words_embs, mask=mask)
        with torch.no_grad(), ops.fixed_order():
            if getattr(netG, "nhwc_out", False):
                return netG(return_nhwc=True, **kw)[1]
            return ops.to_nhwc8(netG(**kw))          # the word-attention generators hand out NCHW f32 only: an exact round trip

    def _chunks(self, n, micro_batch):
        mb = n if not micro_batch else max(1, int(micro_batch))
        return [(i, min(n, i + mb)) for i in range(0, n, mb)]

    def images(self, noise, sent_embs, words_embs=None, mask=None, micro_batch=None):
        """uint8 [n,S,S,3] on the device: trunc((x + 1) * 127.5) of the generator's images, ``micro_batch`` rows per forward (the
        last chunk may be smaller)."""
        out = None
        with _eval_mode(self.netG):
            for i, j in self._chunks(noise.size(0), micro_batch):
                x8 = self.engine_images(noise[i:j], sent_embs[i:j], _rows(words_embs, i, j), _rows(mask, i, j))
                if out is None:
                    out = torch.empty((noise.size(0),) + tuple(x8.shape[1:3]) + (3,), dtype=torch.uint8, device=x8.device)
                ops.image_to_u8(x8, out=out[i:j])
        return out

    def scores(self, x8, sent_embs):
        """the discriminator's conditional logit of engine-layout images for their sentences, f32 [n]: higher = judged more real
        and better matching"""
        if self.netD is None:
            raise ValueError("Sampler.scores needs a discriminator")
        netG, netD = self.netG, self.netD
        with _eval_mode(netD), torch.no_grad(), ops.fixed_order():
            psent = sent_embs if self.separate else netG.proj_sent(sent_embs.float())
            feats = netD(None, nhwc8=x8) if self._d_nhwc else netD(ops.to_nchw(x8, 3))
            return netD.COND_DNET(feats, psent)[0].float().reshape(-1)

    def best_of(self, m, k, noise, sent_embs, words_embs=None, mask=None, micro_batch=None, keep_engine=False):
        """``noise`` [n*m, dim]: rows c*m .. c*m + m - 1 are caption c's m draws.  Every draw is generated and scored; per caption the k
        best are kept.  Returns (uint8 [n,k,S,S,3], scores f32 [n,k] descending, index int64 [n,k] of the kept draws among the m), and
        with ``keep_engine`` as a fourth item the kept images in the engine layout [n*k,S,S,8] (for `ops.image_grid_u8`)."""
        m, k, n = int(m), int(k), sent_embs.size(0)
        if not 1 <= k <= m or noise.size(0) != n * m:
            raise ValueError(f"best_of: 1 <= k <= m and noise of n*m rows expected, got k={k}, m={m}, {noise.size(0)} rows for {n} captions")
        rep = lambda t: None if t is None else t.repeat_interleave(m, dim=0)        # noqa: E731
        sent_r, words_r, mask_r = rep(sent_embs), rep(words_embs), rep(mask)
        u8, x8s, sc = None, [], torch.empty(n * m, dtype=torch.float32, device=self.device)
        with _eval_mode(self.netG):
            for i, j in self._chunks(n * m, micro_batch):
                x8 = self.engine_images(noise[i:j], sent_r[i:j], _rows(words_r, i, j), _rows(mask_r, i, j))
                if u8 is None:
                    u8 = torch.empty((n * m,) + tuple(x8.shape[1:3]) + (3,), dtype=torch.uint8, device=x8.device)
                ops.image_to_u8(x8, out=u8[i:j])
                sc[i:j] = self.scores(x8, sent_r[i:j])
                if keep_engine:
                    x8s.append(x8)
        top, idx = sc.view(n, m).sort(dim=1, descending=True, stable=True)
        top, idx = top[:, :k], idx[:, :k]
        pick = (torch.arange(n, device=idx.device)[:, None] * m + idx).reshape(-1)
        res = (u8[pick].view((n, k) + tuple(u8.shape[1:])), top.contiguous(), idx.contiguous())
        return res + (torch.cat(x8s)[pick],) if keep_engine else res
