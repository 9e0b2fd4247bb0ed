"""The image-image contrastive term of XMC-GAN through a frozen VGG-19 (``TRAIN.ENCODER_LOSS.VGG``).

``VGG19Features`` is torchvision's ``vgg19().features`` in full -- 16 3x3 convolutions with bias and ReLU, five 2x2 max pools -- followed by
the mean over the remaining pixels: one f32 row of 512 numbers per image.  It runs on the engine's layout and in the activation dtype of the
current precision mode: the convolutions through ``ops.conv2d`` (frozen weights: the data gradient only), the ImageNet normalisation and
the fused ReLU + max pool through csrc/vgg.hip.  Which VGG layer XMC-GAN pools is not fixed by the reference (its ``VGG`` switch ends in a
bare ``raise NotImplementedError``): all of ``features``, then the mean, is this project's choice; other layers are not built.
``VGGContrast`` makes the two row sets the loss compares: the real side without a graph, the generated side differentiable.

The weights are a file the user supplies (``--vgg_weights`` / ``XMC_VGG19``): the state dict torchvision ships as ``vgg19-dcbb9e9d.pth``.
They are frozen Parameters held by this object alone -- no module of netG or netD, so nothing of them reaches a checkpoint.

Agreement with torchvision on the real weights file has not been checked (neither is available where this was written); what is checked is
agreement with the plain-torch f64 restatement of the architecture in tests/vgg_ref.py on random weights.
"""
import os

import torch

from . import lib as L
from . import ops
from .ops import ConvGeom

# torchvision's cfg "E": output channels of the 3x3 convolutions (pad 1, bias, ReLU), "M" a 2x2 max pool with stride 2
PLAN = (64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512, "M")
POOLS = PLAN.count("M")
DIMS = 512
WEIGHTS_ENV, WEIGHTS_FLAG = "XMC_VGG19", "--vgg_weights"


def vgg19_layers():
    """[(index in ``features``, cin, cout, a pool follows)] of the convolutions, in forward order: the indices count the ReLU modules
    torchvision puts behind every convolution, which gives 0, 2, 5, 7, 10, ..., 34 for ``PLAN``"""
    out, idx, cin = [], 0, 3
    for k, v in enumerate(PLAN):
        if v == "M":
            idx += 1
            continue
        out.append((idx, cin, v, PLAN[k + 1] == "M"))
        idx, cin = idx + 2, v
    return out


def check_vgg19_state(sd, where):
    """[(weight, bias)] per convolution of a state dict with torchvision's key names, checked against ``PLAN``.  NotImplementedError: a
    ``vgg19_bn`` file; ImportError: a missing key; ValueError: a wrong shape.  ``classifier.*`` is ignored."""
    if any(k.endswith("running_mean") for k in sd):
        raise NotImplementedError(f"VGG19Features: {where} holds BatchNorm statistics (a 'running_mean' key): it is a vgg19_bn file, and "
                                  "only the plain vgg19 (vgg19-dcbb9e9d.pth) is built")
    out = []
    for idx, cin, cout, _ in vgg19_layers():
        got = []
        for key, shape in ((f"features.{idx}.weight", (cout, cin, 3, 3)), (f"features.{idx}.bias", (cout,))):
            if key not in sd:
                raise ImportError(f"VGG19Features: the weights in {where} lack {key!r}")
            if tuple(sd[key].shape) != shape:
                raise ValueError(f"VGG19Features: {key} in {where} is {tuple(sd[key].shape)}, VGG-19 has {shape}")
            got.append(sd[key].detach().to(torch.float32).contiguous())
        out.append(tuple(got))
    return out


def resolve_vgg_weights(given=""):
    """the weights file of the VGG term: ``given`` (the value of --vgg_weights), else $XMC_VGG19.  ImportError without either or without
    the file (refusable before a device is touched)."""
    path = given or os.environ.get(WEIGHTS_ENV, "")
    if not path:
        raise ImportError(f"TRAIN.ENCODER_LOSS.VGG needs torchvision's VGG-19 weights (the vgg19-dcbb9e9d.pth state dict): pass "
                          f"{WEIGHTS_FLAG} PATH or set {WEIGHTS_ENV}.  None is given.")
    if not os.path.isfile(path):
        raise ImportError(f"{WEIGHTS_FLAG}: the VGG-19 weights file {path} does not exist")
    return path


def load_vgg19_weights(path):
    """`check_vgg19_state` of the state dict in ``path``.  ImportError: no file, not a state dict."""
    if not path or not os.path.isfile(path):
        raise ImportError(f"VGG19Features: the weights file {path!r} does not exist ({WEIGHTS_FLAG} PATH or {WEIGHTS_ENV})")
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ImportError(f"VGG19Features: {path} holds a {type(sd).__name__}, a state dict was expected")
    return check_vgg19_state(sd, path)


class VGG19Features:
    """engine image [N,H,W,8] in [-1, 1] -> f32 rows [N,512]; differentiable with respect to the image only."""

    def __init__(self, weights_path, device="cuda"):
        self.device = torch.device(device)
        frozen = lambda t: torch.nn.Parameter(t.to(self.device).contiguous(), requires_grad=False)      # noqa: E731 -- (a Parameter: its packed copy is cached)
        self.layers = [(ConvGeom(cin, cout, 3, 1, 1), frozen(w), frozen(b), pooled)
                       for (_, cin, cout, pooled), (w, b) in zip(vgg19_layers(), load_vgg19_weights(weights_path))]

    def parameters(self):
        return [t for _, w, b, _ in self.layers for t in (w, b)]

    def warm(self):
        """pack every layer's weights for the forward and the data-gradient kernels in the current activation dtype, outside any graph
        capture: a copy packed while a capture records would live in that graph's memory and be packed again at every replay"""
        dt = ops.act_dtype()
        for geom, w, _, _ in self.layers:
            for transpose in (0, 1):
                ops._packed_cached(w, geom, transpose, dt)
        return self

    @staticmethod
    def check_image(x_h, stages=POOLS):
        if x_h.dim() != 4 or x_h.shape[-1] != 8:
            raise ValueError(f"VGG19Features: an engine image [N,H,W,8] expected, got {tuple(x_h.shape)}")
        m = 1 << stages
        if x_h.shape[1] % m or x_h.shape[2] % m or x_h.shape[1] < m or x_h.shape[2] < m:
            raise ValueError(f"VGG19Features: {stages} 2x2 pools need a height and a width that are multiples of {m}, got "
                             f"{x_h.shape[1]}x{x_h.shape[2]}")
        if x_h.dtype != ops.act_dtype():
            raise ValueError(f"VGG19Features: the image is {x_h.dtype}, the {ops.precision()} mode runs on {ops.act_dtype()}")

    def forward(self, x_h, stages=POOLS):
        """``stages``: how many of the five convolution groups run (each ends in its pool) before the mean; the term uses all five, the
        tests also the first two, where the large maps are"""
        self.check_image(x_h, stages)
        ops._need_cuda(x_h)
        x, done = ops.vgg_prep(x_h), 0
        for geom, w, b, pooled in self.layers:
            if done == stages:
                break
            if pooled:
                # max and ReLU commute and this output feeds the pool alone: the raw map is read once forward, and the backward writes
                # the gradient in front of the convolution in one pass (no separate ReLU-mask pass over the network's largest tensors)
                x = ops.relu_maxpool2(ops.conv2d(x, w, b, geom, act=L.ACT_NONE))
                done += 1
            else:
                x = ops.conv2d(x, w, b, geom, act=L.ACT_RELU)
        return ops.global_avgpool(x)

    __call__ = forward


class VGGContrast:
    """the two sides of the VGG term: ``rows(real_h, fake_h)`` -> (real rows without a graph, generated rows with theirs), f32 [N,512] each"""

    def __init__(self, features):
        self.features = features

    def rows(self, real_h, fake_h):
        with torch.no_grad():                # no activation of the real side is kept
            real_rows = self.features(real_h)
        return real_rows, self.features(fake_h)
