"""xmc_gan_amd.ops, layer 4: the leaf nodes.  Pointwise, pooling, layout and augmentation Functions whose backward is written with Functions
of this same module, and from which the later node modules build theirs.  Imports `_config` and `_engine`."""
import torch
from .. import lib as L
from ._config import _code, _need_cuda, _p, _st, fused_blocks
from ._engine import _axpby_bwd_fused, _cast_raw, _zeros_f32_out


# ------------------------------------------------------------------------------------------ pointwise
class CastFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dtype):
        ctx.src = x.dtype
        return _cast_raw(x, dtype)

    @staticmethod
    def backward(ctx, dy):
        return CastFn.apply(dy, ctx.src), None


class MaskFn(torch.autograd.Function):
    """ref > 0 ? dy : slope*dy  (derivative of LeakyReLU/ReLU applied to dy; linear in dy)."""

    @staticmethod
    def forward(ctx, dy, ref, slope):
        dy = dy.contiguous()
        if dy.dtype != ref.dtype:
            dy = dy.to(ref.dtype)
        out = torch.empty_like(dy)
        L.call("xmc_lrelu_mask", _p(dy), _p(ref), _p(out), dy.numel(), float(slope), _code(dy.dtype), _st())
        ctx.slope = slope
        ctx.save_for_backward(ref)
        return out

    @staticmethod
    def backward(ctx, g):
        (ref,) = ctx.saved_tensors
        return MaskFn.apply(g, ref, ctx.slope), None, None


class LreluFn(torch.autograd.Function):
    """nn.LeakyReLU(0.2) (df_gan.py:85,158,214-222,274,277); slope 0 gives nn.ReLU."""

    @staticmethod
    def forward(ctx, x, slope):
        x = x.contiguous()
        y = torch.empty_like(x)
        L.call("xmc_lrelu", _p(x), _p(y), x.numel(), float(slope), _code(x.dtype), _st())
        ctx.slope = slope
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return MaskFn.apply(dy, y, ctx.slope), None


class TanhBwdFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dy, y):
        dy = dy.contiguous()
        if dy.dtype != y.dtype:
            dy = dy.to(y.dtype)
        out = torch.empty_like(dy)
        L.call("xmc_tanh_bwd", _p(dy), _p(y), _p(out), dy.numel(), _code(dy.dtype), _st())
        return out

    @staticmethod
    def backward(ctx, g):
        raise NotImplementedError("second derivative through tanh is not on the XMC-GAN path")


class ScaleFn(torch.autograd.Function):
    """alpha * x with alpha a device scalar (f32 tensor with one element)."""

    @staticmethod
    def forward(ctx, x, alpha):
        x = x.contiguous()
        a = alpha.detach().reshape(-1).float()
        y = torch.empty_like(x)
        L.call("xmc_scale", _p(x), _p(a), _p(y), x.numel(), _code(x.dtype), _st())
        ctx.save_for_backward(x, alpha)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, alpha = ctx.saved_tensors
        dx = ScaleFn.apply(dy, alpha) if ctx.needs_input_grad[0] else None
        da = DotFn.apply(dy, x).reshape(alpha.shape) if ctx.needs_input_grad[1] else None
        return dx, da


class DotFn(torch.autograd.Function):
    """sum(a*b) -> f32 [1]."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = a.contiguous(), b.contiguous()
        if a.dtype != b.dtype:
            b = b.to(a.dtype)
        out = _zeros_f32_out(1, a.device)
        L.call("xmc_dot", _p(a), _p(b), _p(out), a.numel(), _code(a.dtype), _st())
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        da = ScaleFn.apply(b, g) if ctx.needs_input_grad[0] else None
        db = ScaleFn.apply(a, g) if ctx.needs_input_grad[1] else None
        return da, db


class AxpbyFn(torch.autograd.Function):
    """a + alpha*b  (shortcut + gamma*residual, df_gan.py:200,284)."""

    @staticmethod
    def forward(ctx, a, b, alpha):
        a, b = a.contiguous(), b.contiguous()
        al = alpha.detach().reshape(-1).float()
        y = torch.empty_like(a)
        L.call("xmc_axpby", _p(a), _p(b), _p(al), _p(y), a.numel(), _code(a.dtype), _st())
        ctx.save_for_backward(b, alpha)
        return y

    @staticmethod
    def backward(ctx, dy):
        b, alpha = ctx.saved_tensors
        if not torch.is_grad_enabled() and ctx.needs_input_grad[1] and ctx.needs_input_grad[2] and fused_blocks():
            _, db, dal = _axpby_bwd_fused(dy, b, alpha, up=False)
            return (dy if ctx.needs_input_grad[0] else None), db, dal
        da = dy if ctx.needs_input_grad[0] else None
        db = ScaleFn.apply(dy, alpha) if ctx.needs_input_grad[1] else None
        dal = DotFn.apply(dy, b).reshape(alpha.shape) if ctx.needs_input_grad[2] else None
        return da, db, dal


class AxpbyUpFn(torch.autograd.Function):
    """up2(a) + alpha*b without materialising up2(a): the block output `upsample(shortcut) + gamma*residual`."""

    @staticmethod
    def forward(ctx, a, b, alpha, lrelu=False):
        a, b = a.contiguous(), b.contiguous()
        N, H, W, Cc = a.shape
        assert b.shape == (N, 2 * H, 2 * W, Cc)
        al = alpha.detach().reshape(-1).float()
        y = torch.empty_like(b)
        L.call("xmc_axpby_up_lrelu" if lrelu else "xmc_axpby_up", _p(a), _p(b), _p(al), _p(y), N, H, W, Cc, _code(a.dtype), _st())
        ctx.lrelu = lrelu
        ctx.save_for_backward(b, alpha, y if lrelu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        b, alpha, y = ctx.saved_tensors
        if not torch.is_grad_enabled() and all(ctx.needs_input_grad[:3]) and fused_blocks():
            return _axpby_bwd_fused(dy, b, alpha, up=True, ymask=y) + (None,)      # first-order: one pass over dy and b
        if ctx.lrelu:
            dy = MaskFn.apply(dy.contiguous(), y, 0.2)
        da = SumPool2Fn.apply(dy, 1.0) if ctx.needs_input_grad[0] else None
        db = ScaleFn.apply(dy, alpha) if ctx.needs_input_grad[1] else None
        dal = DotFn.apply(dy, b).reshape(alpha.shape) if ctx.needs_input_grad[2] else None
        return da, db, dal, None


# ------------------------------------------------------------------------------------------ reductions, pooling, layout
class ColSumFn(torch.autograd.Function):
    """sum over all pixels -> f32 [C]  (bias gradients)."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        Cc = x.shape[-1]
        out = _zeros_f32_out(Cc, x.device)
        L.call("xmc_colsum", _p(x), _p(out), x.numel() // Cc, Cc, _code(x.dtype), _st())
        ctx.shape, ctx.dtype = x.shape, x.dtype
        return out

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dtype).expand(ctx.shape).contiguous()


class SumPool2Fn(torch.autograd.Function):
    """scale * (2x2 sum pool).  scale=0.25: F.avg_pool2d(x, 2) (df_gan.py:290); adjoint of Up2Fn."""

    @staticmethod
    def forward(ctx, x, scale):
        x = x.contiguous()
        N, H, W, Cc = x.shape
        y = torch.empty((N, H // 2, W // 2, Cc), dtype=x.dtype, device=x.device)
        L.call("xmc_sumpool2", _p(x), _p(y), N, H, W, Cc, float(scale), _code(x.dtype), _st())
        ctx.scale = scale
        return y

    @staticmethod
    def backward(ctx, dy):
        return Up2Fn.apply(dy, ctx.scale), None


class Up2Fn(torch.autograd.Function):
    """scale * nearest x2 upsample.  scale=1: F.interpolate(scale_factor=2) (df_gan.py:202)."""

    @staticmethod
    def forward(ctx, x, scale):
        x = x.contiguous()
        N, H, W, Cc = x.shape
        y = torch.empty((N, 2 * H, 2 * W, Cc), dtype=x.dtype, device=x.device)
        L.call("xmc_upsample2", _p(x), _p(y), N, H, W, Cc, float(scale), _code(x.dtype), _st())
        ctx.scale = scale
        return y

    @staticmethod
    def backward(ctx, dy):
        return SumPool2Fn.apply(dy, ctx.scale), None


class GapFn(torch.autograd.Function):
    """mean over all pixels of an [N,H,W,C] map -> [N,C] (F.avg_pool2d(x,4) on 4x4: df_gan.py:165, train_gan.py:272,275)."""

    @staticmethod
    def forward(ctx, x, out_dtype):
        x = x.contiguous()
        N, H, W, Cc = x.shape
        # (an f32 result is accumulated with atomics on big maps: handed over zero-filled, lib.load() has told the library so)
        y = _zeros_f32_out((N, Cc), x.device) if out_dtype == torch.float32 else torch.empty((N, Cc), dtype=out_dtype, device=x.device)
        L.call("xmc_global_avgpool", _p(x), _p(y), N, H * W, Cc, _code(x.dtype), _code(out_dtype), _st())
        ctx.hw, ctx.dtype = (H, W), x.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        return GapBwdFn.apply(dy, ctx.hw, ctx.dtype), None


class GapBwdFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dy, hw, dtype):
        dy = dy.contiguous()
        N, Cc = dy.shape
        dx = torch.empty((N, hw[0], hw[1], Cc), dtype=dtype, device=dy.device)
        L.call("xmc_global_avgpool_bwd", _p(dy), _p(dx), N, hw[0] * hw[1], Cc, _code(dtype), _code(dy.dtype), _st())
        ctx.in_dtype = dy.dtype
        return dx

    @staticmethod
    def backward(ctx, g):
        return GapFn.apply(g, ctx.in_dtype), None, None


class NchwToNhwc8Fn(torch.autograd.Function):
    """[N,C<=8,H,W] f32 (module boundary, df_gan.py:127) -> [N,H,W,8] activation dtype, zero padded."""

    @staticmethod
    def forward(ctx, x, dtype, out=None):
        _need_cuda(x)
        x = x.contiguous().float()
        N, Cc, H, W = x.shape
        if out is None:
            y = torch.empty((N, H, W, 8), dtype=dtype, device=x.device)
        else:                      # caller-provided destination (e.g. one half of the discriminator's 2B input); written
            # behind autograd's back (no version bump), so it must be a tensor no earlier node has saved
            assert tuple(out.shape) == (N, H, W, 8) and out.dtype == dtype and out.is_contiguous() and out._version == 0
            y = out
        L.call("xmc_nchw_to_nhwc8", _p(x), _p(y), N, Cc, H, W, _code(dtype), _st())
        ctx.c = Cc
        return y

    @staticmethod
    def backward(ctx, dy):
        return Nhwc8ToNchwFn.apply(dy, ctx.c), None, None


class Nhwc8ToNchwFn(torch.autograd.Function):
    """[N,H,W,8] -> [N,C,H,W] f32 (the image NetG returns, df_gan.py:101-103)."""

    @staticmethod
    def forward(ctx, x, c):
        x = x.contiguous()
        N, H, W, _ = x.shape
        y = torch.empty((N, c, H, W), dtype=torch.float32, device=x.device)
        L.call("xmc_nhwc8_to_nchw", _p(x), _p(y), N, c, H, W, _code(x.dtype), _st())
        ctx.dtype = x.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        return NchwToNhwc8Fn.apply(dy, ctx.dtype), None


# ------------------------------------------------------------------------------------------ the frozen VGG-19's pointwise stages
def _vgg_image(x, what):
    _need_cuda(x)
    if x.dim() != 4 or x.shape[-1] != 8:
        raise ValueError(f"{what}: an engine image [N,H,W,8] expected, got {tuple(x.shape)}")
    return x.contiguous()


class VggPrepFn(torch.autograd.Function):
    """((x + 1) / 2 - mean) / std of the engine image [N,H,W,8] in [-1, 1] with torchvision's ImageNet statistics; the five padding channels
    come out zero (xmc_gan_hip.h: xmc_vgg_prep_fwd)."""

    @staticmethod
    def forward(ctx, x):
        x = _vgg_image(x, "vgg_prep")
        y = torch.empty_like(x)
        L.call("xmc_vgg_prep_fwd", _p(x), _p(y), *x.shape[:3], _code(x.dtype), _st())
        return y

    @staticmethod
    def backward(ctx, dy):
        return VggPrepBwdFn.apply(dy)


class VggPrepBwdFn(torch.autograd.Function):
    """dx = dy * 0.5 / std on the three colour channels, zero on the rest; a diagonal map, so it is its own backward."""

    @staticmethod
    def forward(ctx, dy):
        dy = _vgg_image(dy, "vgg_prep backward")
        dx = torch.empty_like(dy)
        L.call("xmc_vgg_prep_bwd", _p(dy), _p(dx), *dy.shape[:3], _code(dy.dtype), _st())
        return dx

    @staticmethod
    def backward(ctx, g):
        return VggPrepBwdFn.apply(g)


class ReluMaxPool2Fn(torch.autograd.Function):
    """F.max_pool2d(F.relu(z), 2) of a raw convolution output z [N,H,W,C] in one pass; the backward writes the gradient in front of the
    convolution in one pass over (z, dp), with torch's tie rule (xmc_gan_hip.h: xmc_relu_maxpool2_bwd)."""

    @staticmethod
    def forward(ctx, z):
        _need_cuda(z)
        z = z.contiguous()
        N, H, W, Cc = z.shape
        p = torch.empty((N, H // 2, W // 2, Cc), dtype=z.dtype, device=z.device)
        L.call("xmc_relu_maxpool2_fwd", _p(z), _p(p), N, H, W, Cc, _code(z.dtype), _st())
        ctx.save_for_backward(z)
        return p

    @staticmethod
    def backward(ctx, dp):
        (z,) = ctx.saved_tensors
        return ReluMaxPool2BwdFn.apply(z, dp)


class ReluMaxPool2BwdFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, dp):
        dp = dp.contiguous()
        if dp.dtype != z.dtype:
            dp = dp.to(z.dtype)
        N, H, W, Cc = z.shape
        dz = torch.empty_like(z)
        L.call("xmc_relu_maxpool2_bwd", _p(z), _p(dp), _p(dz), N, H, W, Cc, _code(z.dtype), _st())
        return dz

    @staticmethod
    def backward(ctx, g):
        raise NotImplementedError("second derivative through relu_maxpool2 is not on the XMC-GAN path")


# ------------------------------------------------------------------------------------------ differentiable augmentation
def _diffaug_raw(x, params, cut, color, channels, transposed, linear_only):
    """one sums launch (only with a colour component) and one apply launch of csrc/augment.hip"""
    _need_cuda(x, params)
    N, H, W, C8 = x.shape
    if C8 != 8 or params.dtype != torch.float32 or tuple(params.shape) != (N, 8) or not params.is_contiguous():
        raise ValueError(f"diffaug: x [N,H,W,8] and params f32 [N,8] expected, got {tuple(x.shape)} and {params.dtype} {tuple(params.shape)}")
    y = torch.empty_like(x)
    dims = (N, H, W, int(channels), int(cut))
    parts = None
    if color:
        parts = torch.empty((N, L.DIFFAUG_PARTS), dtype=torch.float32, device=x.device)
        L.call("xmc_diffaug_sums", _p(x), _p(params), _p(parts), *dims, int(transposed), _code(x.dtype), _st())
    L.call("xmc_diffaug_apply", _p(x), _p(params), _p(parts), _p(y), *dims, int(transposed), int(linear_only), _code(x.dtype), _st())
    return y


class DiffAugFn(torch.autograd.Function):
    """y = A x + (b-term): brightness, saturation, contrast, integer translation with zero fill and cutout of [N,H,W,8] images, per image
    from its row (b, s, c, tx, ty, cy, cx, 0) of the device tensor ``params`` (xmc_gan_hip.h: xmc_diffaug_apply).  ``linear_only``: A x
    alone, the form the backward node's own backward takes.  ``color=False`` promises c == 1 in every row and skips the sums launch."""

    @staticmethod
    def forward(ctx, x, params, cut, color=True, channels=3, linear_only=False):
        x = x.contiguous()
        ctx.params, ctx.args = params, (cut, color, channels)        # (params: a plain attribute, it takes no gradient and the
        return _diffaug_raw(x, params, cut, color, channels, False, linear_only)      # sampler rewrites it in place between iterations)

    @staticmethod
    def backward(ctx, dy):
        dx = DiffAugBwdFn.apply(dy, ctx.params, *ctx.args) if ctx.needs_input_grad[0] else None
        return dx, None, None, None, None, None


class DiffAugBwdFn(torch.autograd.Function):
    """dx = A^T dy (the transposed sums / apply kernels); linear in dy with derivative A, so its backward is `DiffAugFn` without the b-term."""

    @staticmethod
    def forward(ctx, dy, params, cut, color=True, channels=3):
        dy = dy.contiguous()
        ctx.params, ctx.args = params, (cut, color, channels)
        return _diffaug_raw(dy, params, cut, color, channels, True, False)

    @staticmethod
    def backward(ctx, g):
        dg = DiffAugFn.apply(g, ctx.params, *ctx.args, True) if ctx.needs_input_grad[0] else None
        return dg, None, None, None, None
