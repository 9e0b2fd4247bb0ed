"""Plain-torch restatement of xmc_gan_amd/vgg.py for the tests: ImageNet normalisation, the 16 convolutions and five pools of torchvision's
``vgg19().features``, the mean over the pixels -- in f64 (`forward`), in any torch dtype, or in f32 arithmetic with the activations and their
gradients rounded to a 16-bit format after every layer (`emulate`): the yardstick of the 16-bit modes.  NCHW, differentiable.  Also the
pool's backward rule written out by hand, random He-scaled weights, and files in torchvision's key layout."""
import functools

import torch
import torch.nn.functional as F

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
PLAN = (64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512, "M")
CONV_KEYS = (0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28, 30, 32, 34)         # features.<i> of the 16 convolutions


def prep(x):
    """[N,3,H,W] in [-1, 1] -> ((x + 1) / 2 - mean) / std"""
    mean = torch.tensor(MEAN, dtype=x.dtype).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=x.dtype).view(1, 3, 1, 1)
    return ((x + 1) / 2 - mean) / std


def prep_bwd(dy):
    return dy * (0.5 / torch.tensor(STD, dtype=dy.dtype).view(1, 3, 1, 1))


def relu_maxpool2(z):
    """max(0, max of the 2x2 window): [N,C,H,W] -> [N,C,H/2,W/2]"""
    return F.relu(F.max_pool2d(z, 2))


def relu_maxpool2_bwd(z, dp):
    """the rule of xmc_relu_maxpool2_bwd written out: the first position in the scan order (0,0) (0,1) (1,0) (1,1) whose z equals the window's
    maximum gets dp when that maximum is > 0, every other position gets 0"""
    N, C, H, W = z.shape
    win = torch.stack([z[:, :, i::2, j::2] for i in (0, 1) for j in (0, 1)])           # [4,N,C,H/2,W/2] in scan order
    m = win.max(0).values
    taken = torch.zeros_like(m, dtype=torch.bool)
    dz = torch.zeros_like(z)
    for k, (i, j) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        here = (win[k] == m) & ~taken
        taken |= here
        dz[:, :, i::2, j::2] = torch.where(here & (m > 0), dp, torch.zeros_like(dp))
    return dz


def on_16bit_grid(w):
    """``w`` (f64) moved onto values that bf16 AND IEEE half hold exactly: rounded to bf16's 8 significant bits, magnitudes below half's
    smallest normal number (2^-14) set to zero"""
    w = w.to(torch.bfloat16).double()
    return torch.where(w.abs() < 2.0 ** -14, torch.zeros_like(w), w)


def random_weights(seed, grid=True):
    """[(weight [cout,cin,3,3], bias [cout])] in f64: He-scaled weights (variance 2 / fan-in) and biases of +-0.1, so that the activations
    stay of order 1 through all 16 layers.

    ``grid`` (default): the weights lie on values every storage format of the engine holds exactly (`on_16bit_grid`), the biases on f32
    values.  The 16-bit modes keep their convolution weights in the 16-bit format (they are MFMA operands), so weights off that grid are
    rounded once when they are packed.  That is the format's precision, not a kernel's error, and `emulate` -- which rounds activations --
    does not have it.  It matters where rows average many pixels: the weights' rounding is the SAME at every pixel, so the spatial mean
    does not average it away as it does the activations' rounding.  Measured with ``grid=False`` on conv1_1 .. pool2 at 64x64 (a mean over
    256 pixels), max row error / rms: bf16 engine 5.920e-3 against `emulate` 9.16e-4 (x6.5), IEEE half 6.966e-4 against 9.44e-5 (x7.4) --
    and `emulate` on the rounded weights gives 5.920e-3 / 6.98e-4, the engine's figures to three digits.  With the weights on the grid,
    reference, yardstick and engine compute with the same numbers and the comparison is of the kernels.  What the network tests no longer
    see for it is the packing's own rounding of a weight off the grid (to nearest, not truncated; and the low half of a 16-bit weight
    pair, which is identically zero for these weights -- the VGG path uses no pairs).  The convolution tests of tests/test_ops_gpu.py,
    whose weights are off the grid, are what covers that."""
    g = torch.Generator().manual_seed(seed)
    out, cin = [], 3
    for v in PLAN:
        if v == "M":
            continue
        w = torch.randn(v, cin, 3, 3, generator=g, dtype=torch.float64) * (2.0 / (9 * cin)) ** 0.5
        b = (torch.rand(v, generator=g, dtype=torch.float64) - 0.5) * 0.2
        if grid:
            w, b = on_16bit_grid(w), b.float().double()
        out.append((w, b))
        cin = v
    return out


def write_weights_file(path, weights=None, seed=0, drop=(), replace=None):
    """a state dict in torchvision's key layout (f32, with a small ``classifier``, which the loader must ignore) at ``path``.  ``drop``: keys
    left out; ``replace``: {key: tensor} put in or over.  Returns the weights written, as `random_weights` gives them."""
    weights = random_weights(seed) if weights is None else weights
    sd = {}
    for i, (w, b) in zip(CONV_KEYS, weights):
        sd[f"features.{i}.weight"], sd[f"features.{i}.bias"] = w.float(), b.float()
    sd["classifier.0.weight"], sd["classifier.0.bias"] = torch.zeros(4, 8), torch.zeros(4)
    for k in drop:
        del sd[k]
    sd.update(replace or {})
    torch.save(sd, path)
    return weights


class _Round(torch.autograd.Function):
    """the value and its gradient rounded to ``fmt`` (what a tensor stored in that format holds), carried on in the input's dtype"""

    @staticmethod
    def forward(ctx, x, fmt):
        ctx.fmt = fmt
        return x.to(fmt).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.fmt).to(g.dtype), None


def forward(x, weights, stages=5, dtype=torch.float64, fmt=None):
    """[N,3,H,W] in [-1, 1] -> rows [N,C]: prep, the convolution groups up to and including pool number ``stages``, the mean.  Arithmetic
    in ``dtype``; ``fmt``: round every layer's stored tensor (and its gradient) to that format -- prep's output, each ReLU convolution's
    output and the raw output of a convolution in front of a pool (the pool of rounded values is exact)."""
    rnd = (lambda t: t) if fmt is None else (lambda t: _Round.apply(t, fmt))
    h, layer, done = rnd(prep(x.to(dtype))), 0, 0
    for k, v in enumerate(PLAN):
        if done == stages:
            break
        if v == "M":
            continue
        w, b = weights[layer]
        layer += 1
        z = F.conv2d(h, w.to(dtype), b.to(dtype), padding=1)
        if PLAN[k + 1] == "M":
            h = relu_maxpool2(rnd(z))
            done += 1
        else:
            h = rnd(F.relu(z))
    return h.mean((2, 3))


def emulate(fmt):
    """the network in f32 arithmetic with the activations rounded to ``fmt`` (torch.bfloat16 / torch.float16) after every layer"""
    return functools.partial(forward, dtype=torch.float32, fmt=fmt)


def to_engine(x, dtype):
    """[N,3,H,W] -> the engine image [N,H,W,8] in ``dtype``, padding channels zero"""
    N, C, H, W = x.shape
    out = torch.zeros((N, H, W, 8), dtype=dtype)
    out[..., :C] = x.permute(0, 2, 3, 1).to(dtype)
    return out


def from_engine(x_h, c=3):
    """the engine tensor [N,H,W,C8] -> [N,c,H,W] in f64 on the host"""
    return x_h.detach().to("cpu", torch.float64)[..., :c].permute(0, 3, 1, 2).contiguous()
