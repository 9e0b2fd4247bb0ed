"""xmc_gan_amd.ops, layer 3: the leaf nodes.  Pointwise, pooling and layout Functions whose backward is written with Functions of
this same module, and from which the later node modules build theirs.  Imports `_config` and `_engine`."""
import numpy as np
import torch
from .. import lib as L
from ._config import _code, _need_cuda, _p, _st, act_dtype, fused_blocks
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


# ------------------------------------------------------------------------------------------ images as uint8 pixels (csrc/image.hip)
def _image_arg(x8, what):
    """the engine-layout image of the two wrappers below, checked: they are plain functions outside autograd"""
    _need_cuda(x8)
    if x8.dim() != 4 or x8.shape[-1] != 8:
        raise ValueError(f"{what}: an engine-layout image [N,H,W,8] expected, got {tuple(x8.shape)}")
    if x8.requires_grad:
        raise ValueError(f"{what} is not differentiable: detach the image first")
    if x8.dtype != act_dtype():
        raise TypeError(f"{what}: {x8.dtype} image in the {act_dtype()} mode (ops.set_precision)")
    return x8.contiguous()


def _u8_out(out, shape, device, what):
    """the uint8 destination: a new tensor, or the caller's (any byte address: the kernels ask for no alignment of it)"""
    if out is None:
        return torch.empty(shape, dtype=torch.uint8, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != device:
        raise ValueError(f"{what}: out must be a contiguous uint8 {tuple(shape)} tensor on {device}")
    return out


def image_to_u8(x8, out=None):
    """[N,H,W,8] -> uint8 [N,H,W,3] = trunc((x + 1) * 127.5): the bytes of `utils.visual.to_uint8_hwc`, made on the device"""
    x8 = _image_arg(x8, "image_to_u8")
    N, H, W, _ = x8.shape
    y = _u8_out(out, (N, H, W, 3), x8.device, "image_to_u8")
    L.call("xmc_image_to_u8", _p(x8), _p(y), N, H, W, _code(x8.dtype), _st())
    return y


def image_grid_u8(x8, nrow=8, padding=2, out=None):
    """[N,H,W,8] -> uint8 [Hg,Wg,3]: the bytes `utils.visual.save_image(x, normalize=True, scale_each=True)` encodes (every image min-max
    scaled on its own, `nrow` per row, `padding` black pixels around each; one image: the image alone).  Two launches: the per-image
    partial (min, max), then the grid, which writes every byte of it.  ``out``: a contiguous uint8 destination of the grid's size."""
    x8 = _image_arg(x8, "image_grid_u8")
    N, H, W, _ = x8.shape
    nrow, padding = int(nrow), int(padding)
    if nrow < 1 or padding < 0:
        raise ValueError(f"image_grid_u8: nrow {nrow}, padding {padding}")
    pad = 0 if N == 1 else padding
    xmaps = min(nrow, N)
    ymaps = -(-N // xmaps)
    shape = ((H + pad) * ymaps + pad, (W + pad) * xmaps + pad, 3)
    out = _u8_out(out, shape, x8.device, "image_grid_u8")
    parts = torch.empty((N, L.DIFFAUG_PARTS, 2), dtype=torch.float32, device=x8.device)
    L.call("xmc_image_minmax", _p(x8), _p(parts), N, H, W, _code(x8.dtype), _st())
    L.call("xmc_image_grid_u8", _p(x8), _p(parts), _p(out), N, H, W, nrow, padding, _code(x8.dtype), _st())
    return out


# ------------------------------------------------------------------------------------------ training batches from a uint8 image pool (csrc/datafeed.hip)
class HostMirror:
    """A small integer array that lives twice: ``host`` (numpy, drawn or loaded there) and ``dev`` (its device copy, what a kernel reads).
    `crop_flip_normalize` checks the host copy before it launches on the device copy, without a read-back."""

    def __init__(self, host, device=None, dev=None):
        """``device``: upload ``host`` there; or ``dev``: the device copy that already exists (a slice of a larger upload)"""
        self.host = np.ascontiguousarray(host)
        self.dev = torch.from_numpy(self.host).to(device) if dev is None else dev


def validate_crop_params(params, hw, size):
    """The bounds `crop_flip_normalize` needs, checked on host arrays: params int32 [B,4] = (image index, top, left, flip) against
    hw int32 [N,2] = (height, width): 0 <= index < N, 0 <= top <= h - size, 0 <= left <= w - size, flip in {0, 1}.  ValueError names the
    first offending row."""
    params, hw = np.asarray(params), np.asarray(hw)
    if params.ndim != 2 or params.shape[1] != 4 or params.shape[0] < 1 or params.dtype != np.int32:
        raise ValueError(f"crop params: int32 [B,4] with B >= 1 expected, got {params.dtype} {params.shape}")
    if hw.ndim != 2 or hw.shape[1] != 2 or hw.shape[0] < 1 or hw.dtype != np.int32:
        raise ValueError(f"crop params: hw int32 [N,2] with N >= 1 expected, got {hw.dtype} {hw.shape}")
    p = params.astype(np.int64)
    idx, top, left, flip = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    bad = (idx < 0) | (idx >= hw.shape[0])
    h, w = hw[np.where(bad, 0, idx)].astype(np.int64).T
    bad |= (top < 0) | (top > h - size) | (left < 0) | (left > w - size) | (flip < 0) | (flip > 1)
    if bad.any():
        b = int(np.argmax(bad))
        dims = "no such image" if not 0 <= idx[b] < hw.shape[0] else f"image {h[b]} x {w[b]}"
        raise ValueError(f"crop params: row {b} = (index {idx[b]}, top {top[b]}, left {left[b]}, flip {flip[b]}) is out of range for a "
                         f"{size} x {size} crop ({dims}, {hw.shape[0]} images)")


_norm_tables = {}


def normalize_table(device=None):
    """f32 [256]: `xmc_gan.dataset.to_normalized_tensor` of the bytes 0..255, computed by that function on the host (once) and, with a
    ``device``, uploaded (once per device): what `crop_flip_normalize` looks pixels up in"""
    if "host" not in _norm_tables:
        from xmc_gan.dataset import to_normalized_tensor
        _norm_tables["host"] = to_normalized_tensor(np.arange(256, dtype=np.uint8).reshape(16, 16)).reshape(256).contiguous()
    if device is None:
        return _norm_tables["host"]
    key = str(torch.device(device))
    if key not in _norm_tables:
        _norm_tables[key] = _norm_tables["host"].to(device)
    return _norm_tables[key]


def crop_flip_normalize(pool, offsets, hw, params, size, out=None, table=None):
    """B crops out of a device-resident pool of uint8 RGB HWC images -> f32 NCHW [B,3,size,size], the `imgs` of a training step:
    out[b,c,y,x] = table[pool[offsets[i] + ((top + y) * w + left + (flip ? size-1-x : x)) * 3 + c]] with (i, top, left, flip) = params[b].

    ``pool`` uint8 [bytes] (16-byte aligned, a multiple of 16 bytes), ``offsets`` int64 [N], both on the device; ``hw`` a `HostMirror` of
    int32 [N,2] (height, width); ``params`` a `HostMirror` of int32 [B,4], or the host array (uploaded here).  ``table``: f32 [256] on the
    device (default: `normalize_table`).  The host copies are checked (`validate_crop_params`) BEFORE anything is launched; a violation
    is a ValueError.  One launch on the current stream into a new tensor or the caller's ``out``.  size % 8 == 0."""
    if not isinstance(hw, HostMirror):
        raise TypeError("crop_flip_normalize: hw must be an ops.HostMirror (the bounds are checked on its host copy)")
    _need_cuda(pool, offsets, hw.dev)
    if not isinstance(params, HostMirror):
        if torch.is_tensor(params) and params.is_cuda:
            raise TypeError("crop_flip_normalize: params must come with their host copy (an ops.HostMirror or a host array)")
        host = params.numpy() if torch.is_tensor(params) else np.asarray(params)
        validate_crop_params(host, hw.host, int(size))
        params = HostMirror(host, pool.device)
    else:
        validate_crop_params(params.host, hw.host, int(size))
    size, N, B = int(size), hw.host.shape[0], params.host.shape[0]
    if pool.dtype != torch.uint8 or pool.dim() != 1 or not pool.is_contiguous():
        raise ValueError(f"crop_flip_normalize: pool must be a contiguous uint8 vector, got {pool.dtype} {tuple(pool.shape)}")
    if offsets.dtype != torch.int64 or tuple(offsets.shape) != (N,) or not offsets.is_contiguous():
        raise ValueError(f"crop_flip_normalize: offsets int64 [{N}] expected, got {offsets.dtype} {tuple(offsets.shape)}")
    if hw.dev.dtype != torch.int32 or params.dev.dtype != torch.int32 or tuple(params.dev.shape) != (B, 4) or tuple(hw.dev.shape) != (N, 2):
        raise ValueError("crop_flip_normalize: the device copies of hw / params do not match their host copies")
    table = normalize_table(pool.device) if table is None else table
    _need_cuda(table, params.dev)
    if table.dtype != torch.float32 or table.numel() != 256 or not table.is_contiguous():
        raise ValueError("crop_flip_normalize: table must be a contiguous f32 [256]")
    shape = (B, 3, size, size)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=pool.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != pool.device:
        raise ValueError(f"crop_flip_normalize: out must be a contiguous f32 {shape} tensor on {pool.device}")
    L.call("xmc_crop_flip_normalize", _p(pool), pool.numel(), _p(offsets), _p(hw.dev), N, _p(params.dev), _p(table), _p(out), B, size, _st())
    return out


# ------------------------------------------------------------------------------------------ a batch's text-encoder outputs from cached embeddings (csrc/captionfeed.hip)
def validate_caption_rows(rows, n):
    """The bound `caption_gather` needs, checked on the host array: rows int32 [B], B >= 1, every entry in [0, n).  ValueError names the
    first offending entry."""
    rows = np.asarray(rows)
    if rows.ndim != 1 or rows.shape[0] < 1 or rows.dtype != np.int32:
        raise ValueError(f"caption rows: int32 [B] with B >= 1 expected, got {rows.dtype} {rows.shape}")
    bad = (rows < 0) | (rows >= n)
    if bad.any():
        b = int(np.argmax(bad))
        raise ValueError(f"caption rows: entry {b} = {int(rows[b])} is out of range for a table of {n} captions")


def caption_gather(sent_tab, tok_tab, tok_offsets, lens, rows, T, out=None):
    """What a frozen text encoder returned for the captions ``rows`` when the tables were written: (words_embs f32 [B,E,T], sent_embs f32
    [B,E], mask bool [B,T], True at padding), one launch on the current stream.  words_embs[b,e,t] = tok_tab[tok_offsets[r] + t, e] for
    t < lens[r] and 0 beyond, sent_embs[b] = sent_tab[r], r = rows[b].

    ``sent_tab`` f32 [N,E], ``tok_tab`` f32 [rows,E] (only the valid tokens, caption by caption), ``tok_offsets`` int64 [N], ``lens`` int32 [N],
    all on the device; ``rows`` a `HostMirror` of int32 [B], or the host array (uploaded here).  The host copy is checked
    (`validate_caption_rows`) BEFORE anything is launched; a violation, or rows that come without a host copy, is a ValueError.  ``out``: the
    caller's three tensors.  E % 4 == 0, 1 <= T <= 64: anything else is the library's XMC_ESHAPE, raised as ValueError."""
    N = int(lens.shape[0]) if lens.dim() == 1 else -1
    if isinstance(rows, HostMirror):
        validate_caption_rows(rows.host, N)
    else:
        if torch.is_tensor(rows):
            if rows.device.type != "cpu":
                raise ValueError("caption_gather: rows must come with their host copy (an ops.HostMirror or a host array): the bound is "
                                 "checked there, without a read-back")
            rows = rows.numpy()
        validate_caption_rows(rows, N)
        _need_cuda(sent_tab)
        rows = HostMirror(rows, sent_tab.device)
    _need_cuda(sent_tab, tok_tab, tok_offsets, lens, rows.dev)
    T, B = int(T), rows.host.shape[0]
    if sent_tab.dtype != torch.float32 or sent_tab.dim() != 2 or sent_tab.shape[0] != N or not sent_tab.is_contiguous():
        raise ValueError(f"caption_gather: sent_tab must be a contiguous f32 [{N},E] tensor, got {sent_tab.dtype} {tuple(sent_tab.shape)}")
    E = int(sent_tab.shape[1])
    if tok_tab.dtype != torch.float32 or tok_tab.dim() != 2 or tok_tab.shape[1] != E or tok_tab.shape[0] < 1 or not tok_tab.is_contiguous():
        raise ValueError(f"caption_gather: tok_tab must be a contiguous f32 [rows >= 1,{E}] tensor, got {tok_tab.dtype} {tuple(tok_tab.shape)}")
    if tok_offsets.dtype != torch.int64 or tuple(tok_offsets.shape) != (N,) or not tok_offsets.is_contiguous() or lens.dtype != torch.int32 \
            or not lens.is_contiguous():
        raise ValueError(f"caption_gather: tok_offsets int64 [{N}] and lens int32 [{N}] expected, got {tok_offsets.dtype} "
                         f"{tuple(tok_offsets.shape)} and {lens.dtype} {tuple(lens.shape)}")
    if rows.dev.dtype != torch.int32 or tuple(rows.dev.shape) != (B,) or not rows.dev.is_contiguous():
        raise ValueError("caption_gather: the device copy of rows does not match its host copy")
    dev = sent_tab.device
    shapes = ((B, E, T), (B, E), (B, T))
    dtypes = (torch.float32, torch.float32, torch.bool)
    if out is None:
        out = tuple(torch.empty(s, dtype=d, device=dev) for s, d in zip(shapes, dtypes))
    elif len(out) != 3 or any(tuple(o.shape) != s or o.dtype != d or not o.is_contiguous() or o.device != dev for o, s, d in zip(out, shapes, dtypes)):
        raise ValueError(f"caption_gather: out must be contiguous f32 {shapes[0]}, f32 {shapes[1]} and bool {shapes[2]} tensors on {dev}")
    words, sent, mask = out
    rc = getattr(L.load(), "xmc_caption_gather")(_p(sent_tab), _p(tok_tab), tok_tab.shape[0], _p(tok_offsets), _p(lens), N, _p(rows.dev), B, E, T,
                                                 _p(words), _p(sent), _p(mask), _st())
    if rc == -3:
        raise ValueError(f"caption_gather: XMC_ESHAPE (shape out of range): E = {E} must be a multiple of 4 and T = {T} in [1, 64]")
    L.check(rc, "xmc_caption_gather")
    return words, sent, mask


# ------------------------------------------------------------------------------------------ FID evaluation (csrc/fid.hip): f32, outside autograd
def _fid_arg(x, what, dtype, dims):
    _need_cuda(x)
    if x.dim() != dims or x.dtype != dtype or x.requires_grad:
        raise ValueError(f"{what}: a {dims}-d {dtype} tensor without a gradient expected, got {tuple(x.shape)} {x.dtype}")
    return x.contiguous()


def fid_resize_u8(u8, out_hw=None):
    """uint8 [N,H,W,3] (what `image_to_u8` writes and PIL reads) -> f32 engine image [N,OH,OW,8]: bilinear (align_corners=False, no
    antialias) to ``out_hw`` (None: the size it has), then 2 * (x / 255) - 1; channels 3..7 are zero"""
    u8 = _fid_arg(u8, "fid_resize_u8", torch.uint8, 4)
    N, H, W, c = u8.shape
    if c != 3 or N < 1 or H < 1 or W < 1:
        raise ValueError(f"fid_resize_u8: uint8 [N,H,W,3] expected, got {tuple(u8.shape)}")
    OH, OW = (H, W) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
    if OH < 1 or OW < 1:
        raise ValueError(f"fid_resize_u8: output size {OH}x{OW}")
    y = torch.empty((N, OH, OW, 8), dtype=torch.float32, device=u8.device)
    L.call("xmc_fid_resize_u8", _p(u8), _p(y), N, H, W, OH, OW, _st())
    return y


_POOL_MODES = {"max": L.POOL_MAX, "avg": L.POOL_AVG_VALID, "avg_pad": L.POOL_AVG_PAD}


def resize_bilinear_f32(x, out_hw=None):
    """f32 NCHW [N,3,H,W] (what a generator returns) -> f32 engine image [N,OH,OW,8]: bilinear (align_corners=False, no antialias) to
    ``out_hw`` (None: the size it has) by `fid_resize_u8`'s coordinate rule, values not rescaled; channels 3..7 are zero"""
    x = _fid_arg(x, "resize_bilinear_f32", torch.float32, 4)
    N, c, H, W = x.shape
    if c != 3 or N < 1 or H < 1 or W < 1:
        raise ValueError(f"resize_bilinear_f32: f32 [N,3,H,W] expected, got {tuple(x.shape)}")
    OH, OW = (H, W) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
    if OH < 1 or OW < 1:
        raise ValueError(f"resize_bilinear_f32: output size {OH}x{OW}")
    y = torch.empty((N, OH, OW, 8), dtype=torch.float32, device=x.device)
    L.call("xmc_resize_bilinear_f32", _p(x), _p(y), N, H, W, OH, OW, _st())
    return y


def pool3x3(x, mode, stride):
    """3x3 pool of f32 [N,H,W,C] (C % 4 == 0).  ``mode`` 'max', 'avg' (the sum over the window's in-image pixels divided by their number:
    avg_pool2d(count_include_pad=False)) or 'avg_pad' (the same sum / 9: count_include_pad=True; stride 1 only); ``stride`` 1 (padding 1,
    same size) or 2 (no padding, floor((H - 3) / 2) + 1 rows)"""
    x = _fid_arg(x, "pool3x3", torch.float32, 4)
    if mode not in _POOL_MODES or stride not in (1, 2) or (mode == "avg_pad" and stride != 1):
        raise ValueError(f"pool3x3: mode {mode!r}, stride {stride}")
    N, H, W, Cc = x.shape
    if N < 1 or Cc < 4 or Cc % 4 or H < 1 or W < 1 or (stride == 2 and (H < 3 or W < 3)):
        raise ValueError(f"pool3x3: {tuple(x.shape)} at stride {stride} (C % 4 == 0; stride 2 needs a whole 3x3 window)")
    OH, OW = (H, W) if stride == 1 else ((H - 3) // 2 + 1, (W - 3) // 2 + 1)
    y = torch.empty((N, OH, OW, Cc), dtype=torch.float32, device=x.device)
    L.call("xmc_pool3x3", _p(x), _p(y), N, H, W, Cc, _POOL_MODES[mode], stride, _st())
    return y


def fid_moments(feats, total, outer):
    """total f64 [D] += column sums of feats f32 [B,D]; outer f64 [D,D] += feats^T feats, in f64 and in a fixed order (same bytes every run)"""
    feats = _fid_arg(feats, "fid_moments", torch.float32, 2)
    B, D = feats.shape
    for t, shape in ((total, (D,)), (outer, (D, D))):
        _need_cuda(t)
        if t.dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != feats.device:
            raise ValueError(f"fid_moments: accumulator {tuple(t.shape)} {t.dtype}, a contiguous f64 {shape} on {feats.device} expected")
    if B < 1:
        raise ValueError("fid_moments: an empty batch")
    L.call("xmc_fid_moments", _p(feats), _p(total), _p(outer), B, D, _st())


# ------------------------------------------------------------------------------------------ R-precision (csrc/retrieval.hip): f32, outside autograd
def rprecision(img, txt, cand, return_scores=False):
    """Caption retrieval among K candidates per image: img f32 [N,D] image codes, txt f32 [M,D] caption codes, cand int32 [N,K] rows of
    ``txt`` (column 0: the image's own caption) -> rank int32 [N], the number of other candidates whose cosine beats the own caption's
    (0: a hit; K: the own caption scored NaN); ``return_scores``: (rank, score f32 [N,K]).  D % 4 == 0, D <= 1024.  ``cand`` is checked
    against [0, M) here, on the host (one synchronising reduction when it lives on the device)."""
    img, txt = _fid_arg(img, "rprecision", torch.float32, 2), _fid_arg(txt, "rprecision", torch.float32, 2)
    cand = torch.as_tensor(cand)
    if cand.dim() != 2 or cand.dtype != torch.int32:
        raise ValueError(f"rprecision: cand int32 [N,K] expected, got {cand.dtype} {tuple(cand.shape)}")
    (N, D), (M, D2), K = img.shape, txt.shape, cand.shape[1]
    if D != D2 or cand.shape[0] != N or N < 1 or M < 1 or K < 1 or txt.device != img.device:
        raise ValueError(f"rprecision: img {tuple(img.shape)}, txt {tuple(txt.shape)}, cand {tuple(cand.shape)} do not fit")
    if D % 4 or D > 1024:
        raise ValueError(f"rprecision: D = {D}; D % 4 == 0 and D <= 1024 expected")
    lo, hi = int(cand.min()), int(cand.max())
    if lo < 0 or hi >= M:
        raise ValueError(f"rprecision: candidate indices span [{lo}, {hi}], txt has {M} rows")
    cand = cand.to(img.device).contiguous()
    rank = torch.empty((N,), dtype=torch.int32, device=img.device)
    score = torch.empty((N, K), dtype=torch.float32, device=img.device) if return_scores else None
    L.call("xmc_rprecision", _p(img), _p(txt), _p(cand), _p(rank), _p(score), N, M, K, D, _st())
    return (rank, score) if return_scores else rank


# ------------------------------------------------------------------------------------------ precision / recall / density / coverage (csrc/manifold.hip): f32, outside autograd
def _manifold_dims(what, *xs):
    D = xs[0].shape[1]
    if any(x.shape[1] != D or x.shape[0] < 1 or x.device != xs[0].device for x in xs) or D < 4 or D % 4 or D > 4096:
        raise ValueError(f"{what}: f32 [N,D] rows on one device with D % 4 == 0 and 4 <= D <= 4096 expected, got {[tuple(x.shape) for x in xs]}")
    return D


def _manifold_slices(what, nq, nc, slices):
    slices = int(slices)
    if slices < 0:
        raise ValueError(f"{what}: slices = {slices}")
    return getattr(L.load(), "xmc_manifold_slices")(nq, nc, slices)


def row_sqnorm(x):
    """|x_i|^2 of the rows of x f32 [N,D] (D % 4 == 0, D <= 4096) -> f32 [N], summed in a fixed order"""
    x = _fid_arg(x, "row_sqnorm", torch.float32, 2)
    D = _manifold_dims("row_sqnorm", x)
    n2 = torch.empty((x.shape[0],), dtype=torch.float32, device=x.device)
    L.call("xmc_row_sqnorm", _p(x), _p(n2), x.shape[0], D, _st())
    return n2


def knn_radius2(x, k, slices=0):
    """rad2 f32 [N]: the k-th smallest squared distance from row i of x f32 [N,D] to the OTHER rows (excluded by index; duplicates are
    neighbours at distance 0).  1 <= k <= 16, N >= k + 1.  ``slices``: ranges the candidate rows are split into (0: the library
    chooses); the result is the same bytes for every value."""
    x = _fid_arg(x, "knn_radius2", torch.float32, 2)
    D, N, k = _manifold_dims("knn_radius2", x), x.shape[0], int(k)
    if not 1 <= k <= 16 or N < k + 1:
        raise ValueError(f"knn_radius2: k = {k} with {N} rows; 1 <= k <= 16 and N >= k + 1 expected")
    S = _manifold_slices("knn_radius2", N, N, slices)
    n2 = row_sqnorm(x)
    r2 = torch.empty((N,), dtype=torch.float32, device=x.device)
    ws = torch.empty((S * N * k,), dtype=torch.float32, device=x.device) if S > 1 else None
    L.call("xmc_knn_radius2", _p(x), _p(n2), _p(r2), _p(ws), 0 if ws is None else ws.numel() * 4, N, D, k, S, _st())
    return r2


def manifold_count(a, b, rb2, slices=0):
    """For every row i of a f32 [Na,D] against the rows of b f32 [Nb,D]: count int32 [Na] = the number of rows j of b with
    |a_i - b_j|^2 <= rb2[j] (rb2 f32 [Nb], e.g. `knn_radius2(b, k)`), and near2 f32 [Na] = min_j |a_i - b_j|^2.  ``rb2`` None: count is
    None and only near2 is computed.  Returns (count, near2); the same bytes for every ``slices``."""
    a, b = _fid_arg(a, "manifold_count", torch.float32, 2), _fid_arg(b, "manifold_count", torch.float32, 2)
    D, Na, Nb = _manifold_dims("manifold_count", a, b), a.shape[0], b.shape[0]
    if rb2 is not None:
        rb2 = _fid_arg(rb2, "manifold_count", torch.float32, 1)
        if rb2.shape[0] != Nb or rb2.device != a.device:
            raise ValueError(f"manifold_count: rb2 {tuple(rb2.shape)} on {rb2.device}, f32 [{Nb}] on {a.device} expected")
    S = _manifold_slices("manifold_count", Na, Nb, slices)
    na2, nb2 = row_sqnorm(a), row_sqnorm(b)
    count = torch.empty((Na,), dtype=torch.int32, device=a.device) if rb2 is not None else None
    near2 = torch.empty((Na,), dtype=torch.float32, device=a.device)
    ws = torch.empty((S * Na * 2,), dtype=torch.float32, device=a.device) if S > 1 else None
    L.call("xmc_manifold_count", _p(a), _p(na2), _p(b), _p(nb2), _p(rb2), _p(count), _p(near2), _p(ws), 0 if ws is None else ws.numel() * 4,
           Na, Nb, D, S, _st())
    return count, near2


# ------------------------------------------------------------------------------------------ KID / Inception Score (csrc/kid.hip): outside autograd
def _index_table(what, idx, n, device):
    """an int32 [S,m] table of rows of a bank of ``n`` rows, checked against [0, n) HERE, on the host, before anything is launched"""
    idx = torch.as_tensor(idx)
    if idx.dim() != 2 or idx.dtype != torch.int32 or idx.shape[0] < 1:
        raise ValueError(f"{what}: an int32 [S,m] index table expected, got {idx.dtype} {tuple(idx.shape)}")
    if idx.numel():
        lo, hi = int(idx.min()), int(idx.max())
        if lo < 0 or hi >= n:
            raise ValueError(f"{what}: the indices span [{lo}, {hi}], the bank has {n} rows")
    return idx.to(device).contiguous()


def poly_mmd_sums(real, fake, idx_real, idx_fake):
    """The kernel sums of KID's unbiased MMD^2, k(x, y) = (x.y / D + 1)^3, for S subsets of m rows per side in one launch: real f32 [Nr,D],
    fake f32 [Nf,D], idx_real / idx_fake int32 [S,m] (rows of the banks, checked against them on the host) -> f64 [S,3]: the sum of k over
    the ordered pairs i != j (by POSITION in the subset) of the real subset, the same of the generated one, and the sum over all m^2 cross
    pairs.  D % 4 == 0, 4 <= D <= 4096, m >= 2.  No m x m matrix and no gathered copy of a subset is stored; the same bytes every run."""
    real, fake = _fid_arg(real, "poly_mmd_sums", torch.float32, 2), _fid_arg(fake, "poly_mmd_sums", torch.float32, 2)
    D = _manifold_dims("poly_mmd_sums", real, fake)
    ir, jf = _index_table("poly_mmd_sums", idx_real, real.shape[0], real.device), _index_table("poly_mmd_sums", idx_fake, fake.shape[0], real.device)
    (S, m) = ir.shape
    if tuple(jf.shape) != (S, m) or m < 2 or S > 65535:
        raise ValueError(f"poly_mmd_sums: index tables {tuple(ir.shape)} and {tuple(jf.shape)}; two [S,m] tables with m >= 2 and S <= 65535 expected")
    tiles = getattr(L.load(), "xmc_poly_mmd_tiles")(m)
    out = torch.empty((S, 3), dtype=torch.float64, device=real.device)
    ws = torch.empty((S * tiles,), dtype=torch.float64, device=real.device)
    L.call("xmc_poly_mmd_sums", _p(real), _p(fake), _p(ir), _p(jf), _p(out), _p(ws), ws.numel() * 8, real.shape[0], fake.shape[0], D, S, m, _st())
    return out


def inception_score_sums(logits, splits, classes=None):
    """logits f32 [N,ld] (``classes``: only the first that many columns are logits, the others are never read) cut into ``splits``
    consecutive parts [s N // splits, (s + 1) N // splits) -> (H f64 [splits], P f64 [splits,C]): per part the sum of p log p over rows and
    classes and the per-class sum of p over rows, p = softmax(row), everything in f64 and in a fixed order.  C <= 1024, 1 <= splits <= N."""
    _need_cuda(logits)
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.requires_grad or logits.stride(1) != 1 or logits.stride(0) < logits.shape[1]:
        raise ValueError(f"inception_score_sums: f32 logits [N,C] with unit column stride expected, got {logits.dtype} {tuple(logits.shape)}")
    N, C, splits = logits.shape[0], int(logits.shape[1] if classes is None else classes), int(splits)
    if not 1 <= C <= min(1024, logits.shape[1]) or not 1 <= splits <= min(N, 65535):
        raise ValueError(f"inception_score_sums: {N} rows, {C} of {logits.shape[1]} columns, {splits} splits; 1 <= C <= 1024 and 1 <= splits <= N expected")
    H = torch.empty((splits,), dtype=torch.float64, device=logits.device)
    P = torch.empty((splits, C), dtype=torch.float64, device=logits.device)
    nbytes = getattr(L.load(), "xmc_inception_score_ws_bytes")(N, C, splits)
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=logits.device)
    L.call("xmc_inception_score", _p(logits), logits.stride(0), _p(H), _p(P), _p(ws), nbytes, N, C, splits, _st())
    return H, P


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
