"""Fréchet Inception Distance on the device: what the reference leaves to ``pytorch_fid`` (train_gan.py:389,
``calculate_fid_given_paths([org_dir, save_dir], batch_size=100, dims=2048)``).

``InceptionFID`` is the FID variant of Inception-v3 up to its 2048-d pooled features, run in f32 on this package's kernels whatever
``ops.set_precision`` says: the 94 convolutions (BatchNorm folded in, ReLU in the epilogue) through ``xmc_conv_igemm``'s tap tables, the
image front end, the 3x3 pools and the f64 feature moments through csrc/fid.hip.  The weights are a file the user supplies
(``weights=`` / ``XMC_FID_INCEPTION``): the ``pt_inception-2015-12-05-*.pth`` state dict of pytorch_fid, torchvision key names.
The layers, blocks and trunk live in ``InceptionTrunk``, which also runs torchvision's flavour of the network (``variant="torchvision"``:
the trunk of the DAMSM image encoder, xmc_gan_amd/rprecision.py).  ``FeatureStats`` accumulates mean and covariance on the device in f64; ``frechet_distance`` is host f64 numpy (two symmetric
eigendecompositions and one SVD, no scipy).  Statistics files are pytorch_fid's ``.npz`` (``mu``, ``sigma``).

Agreement with pytorch_fid on the real weights file has not been checked (neither is available where this was written); what is checked is
agreement with the plain-torch f64 restatement of the architecture in tests/fid_ref.py.
"""
import os

import numpy as np
import torch

from . import lib as L
from . import ops
from .ops import ConvGeom, _conv_fwd_raw

BN_EPS = 1e-3
DIMS = 2048
CLASSES = 1008            # the outputs of the 2015 Inception's ``fc``: all of them enter the Inception Score
IS_SPLITS = 10
IMAGE_EXTENSIONS = (".png", ".jpg", ".jpeg")


def inception_layers():
    """{layer name: (cin, cout, (kh, kw), stride, (ph, pw))} of the 94 BasicConv2d (conv without bias -> BatchNorm -> ReLU), in forward order"""
    t = {}

    def c(name, cin, cout, k=1, s=1, p=0):
        t[name] = (cin, cout, (k, k) if isinstance(k, int) else k, s, (p, p) if isinstance(p, int) else p)

    c("Conv2d_1a_3x3", 3, 32, 3, 2)
    c("Conv2d_2a_3x3", 32, 32, 3)
    c("Conv2d_2b_3x3", 32, 64, 3, 1, 1)
    c("Conv2d_3b_1x1", 64, 80)
    c("Conv2d_4a_3x3", 80, 192, 3)
    for m, cin, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        c(m + ".branch1x1", cin, 64)
        c(m + ".branch5x5_1", cin, 48)
        c(m + ".branch5x5_2", 48, 64, 5, 1, 2)
        c(m + ".branch3x3dbl_1", cin, 64)
        c(m + ".branch3x3dbl_2", 64, 96, 3, 1, 1)
        c(m + ".branch3x3dbl_3", 96, 96, 3, 1, 1)
        c(m + ".branch_pool", cin, pf)
    c("Mixed_6a.branch3x3", 288, 384, 3, 2)
    c("Mixed_6a.branch3x3dbl_1", 288, 64)
    c("Mixed_6a.branch3x3dbl_2", 64, 96, 3, 1, 1)
    c("Mixed_6a.branch3x3dbl_3", 96, 96, 3, 2)
    for m, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        c(m + ".branch1x1", 768, 192)
        c(m + ".branch7x7_1", 768, c7)
        c(m + ".branch7x7_2", c7, c7, (1, 7), 1, (0, 3))
        c(m + ".branch7x7_3", c7, 192, (7, 1), 1, (3, 0))
        c(m + ".branch7x7dbl_1", 768, c7)
        c(m + ".branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0))
        c(m + ".branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3))
        c(m + ".branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0))
        c(m + ".branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3))
        c(m + ".branch_pool", 768, 192)
    c("Mixed_7a.branch3x3_1", 768, 192)
    c("Mixed_7a.branch3x3_2", 192, 320, 3, 2)
    c("Mixed_7a.branch7x7x3_1", 768, 192)
    c("Mixed_7a.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3))
    c("Mixed_7a.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0))
    c("Mixed_7a.branch7x7x3_4", 192, 192, 3, 2)
    for m, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        c(m + ".branch1x1", cin, 320)
        c(m + ".branch3x3_1", cin, 384)
        c(m + ".branch3x3_2a", 384, 384, (1, 3), 1, (0, 1))
        c(m + ".branch3x3_2b", 384, 384, (3, 1), 1, (1, 0))
        c(m + ".branch3x3dbl_1", cin, 448)
        c(m + ".branch3x3dbl_2", 448, 384, 3, 1, 1)
        c(m + ".branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1))
        c(m + ".branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0))
        c(m + ".branch_pool", cin, 192)
    return t


BLOCKS = ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7a", "Mixed_7b", "Mixed_7c")
BLOCK_IN = dict(Mixed_5b=192, Mixed_5c=256, Mixed_5d=288, Mixed_6a=288, Mixed_6b=768, Mixed_6c=768, Mixed_6d=768, Mixed_6e=768,
                Mixed_7a=768, Mixed_7b=1280, Mixed_7c=2048)


def fold_bn(w, gamma, beta, mean, var, eps=BN_EPS):
    """conv (no bias) followed by an evaluation-mode BatchNorm as one convolution with a bias: f64 on the host, f32 results"""
    w, gamma, beta, mean, var = (t.detach().to("cpu", torch.float64) for t in (w, gamma, beta, mean, var))
    scale = gamma / torch.sqrt(var + eps)
    return (w * scale[:, None, None, None]).float().contiguous(), (beta - mean * scale).float().contiguous()


def check_inception_state(sd, who, where):
    """{layer: (weight, gamma, beta, running_mean, running_var)} of a state dict with torchvision's Inception-v3 key names, checked against
    `inception_layers()`.  ImportError: a missing key; ValueError: a wrong shape.  Other keys are ignored."""
    out = {}
    for name, (cin, cout, (kh, kw), _, _) in inception_layers().items():
        keys = [(f"{name}.conv.weight", (cout, cin, kh, kw))] + [(f"{name}.bn.{k}", (cout,)) for k in ("weight", "bias", "running_mean", "running_var")]
        got = []
        for key, shape in keys:
            if key not in sd:
                raise ImportError(f"{who}: the weights in {where} lack {key!r}")
            if tuple(sd[key].shape) != shape:
                raise ValueError(f"{who}: {key} is {tuple(sd[key].shape)}, Inception-v3 has {shape}")
            got.append(sd[key])
        out[name] = tuple(got)
    return out


def load_inception_weights(path=None):
    """The FID Inception state dict of ``path`` (default: $XMC_FID_INCEPTION), checked against `inception_layers()`: {layer: (weight,
    gamma, beta, running_mean, running_var)}.  ``fc.*`` and ``num_batches_tracked`` are ignored.  ImportError: no path, no file, a
    missing key; ValueError: a wrong shape."""
    path = path or os.environ.get("XMC_FID_INCEPTION", "")
    if not path:
        raise ImportError(
            "InceptionFID needs the FID Inception weights (the pt_inception-2015-12-05-*.pth state dict that pytorch_fid downloads): pass "
            "weights= / --fid_inception / --inception or set XMC_FID_INCEPTION.  None is given.")
    if not os.path.isfile(path):
        raise ImportError(f"InceptionFID: the weights file {path} does not exist")
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ImportError(f"InceptionFID: {path} holds a {type(sd).__name__}, a state dict was expected")
    return check_inception_state(sd, "InceptionFID", path)


def load_inception_fc(path=None):
    """``fc.weight`` f32 [1008, 2048] of the same file `load_inception_weights` reads (the classifier of the Inception Score; its bias is
    not used).  ImportError: no path or no file; ValueError: the file holds no such tensor, or one of another shape."""
    path = path or os.environ.get("XMC_FID_INCEPTION", "")
    if not path or not os.path.isfile(path):
        raise ImportError(f"the Inception Score needs the FID Inception weights file, got {path!r}")
    sd = torch.load(path, map_location="cpu", weights_only=True)
    w = sd.get("fc.weight") if isinstance(sd, dict) else None
    if w is None:
        raise ValueError(f"the weights in {path} hold no 'fc.weight' (the [{CLASSES}, {DIMS}] classifier the Inception Score takes its logits from)")
    if tuple(w.shape) != (CLASSES, DIMS):
        raise ValueError(f"fc.weight in {path} is {tuple(w.shape)}, the Inception Score needs [{CLASSES}, {DIMS}]")
    return w.detach().to(torch.float32).contiguous()


def conv_bias_relu(x, w, b, geom):
    """relu(conv(x, w) + b) in f32 on the generic implicit-GEMM kernel: x f32 [N,H,W,cin (3 -> 8)], w [cout,cin,kh,kw], b f32 [cout].
    A kernel of more than MAX_TAPS taps (the 5x5 layers: 25) runs as tap ranges, each added to the one before in f32, then the ReLU."""
    if geom.ntaps <= L.MAX_TAPS:
        return _conv_fwd_raw(x, w, b, geom, L.ACT_RELU, torch.float32)
    y = None
    for lo in range(0, geom.ntaps, L.MAX_TAPS):
        y = _conv_fwd_raw(x, w, b if y is None else None, geom, L.ACT_NONE, torch.float32, res=y, taps=(lo, min(geom.ntaps, lo + L.MAX_TAPS)))
    out = torch.empty_like(y)
    L.call("xmc_lrelu", ops._p(y), ops._p(out), y.numel(), 0.0, L.F32, ops._st())          # slope 0: a ReLU
    return out


VARIANTS = ("fid", "torchvision")


class InceptionTrunk:
    """The 94 folded convolutions of Inception-v3 and its blocks, on f32 engine tensors [N,H,W,C].  ``raw``: what `load_inception_weights`
    returns.  ``variant`` "fid": pytorch_fid's network (pool branches average over the in-image pixels, Mixed_7c's is a max pool);
    "torchvision": every ``branch_pool`` is avg_pool2d(3, 1, 1) with its default count_include_pad=True -- the sum / 9 -- Mixed_7c's
    included (the network AttnGAN's DAMSM image encoder was trained on: xmc_gan/model/encoder.py CNN_ENCODER)."""

    def __init__(self, raw, device="cuda", variant="fid"):
        if variant not in VARIANTS:
            raise ValueError(f"InceptionTrunk: variant {variant!r}, one of {VARIANTS} expected")
        self.device = torch.device(device)
        self.variant = variant
        self.layers = {}
        for name, (cin, cout, k, s, p) in inception_layers().items():
            w, b = fold_bn(*raw[name])
            frozen = lambda t: torch.nn.Parameter(t.to(self.device).contiguous(), requires_grad=False)      # noqa: E731 -- (a Parameter: its packed copy is cached)
            self.layers[name] = (ConvGeom(cin, cout, k, s, p), frozen(w), frozen(b))

    # ---- layers
    def conv(self, name, x):
        """BasicConv2d `name` on f32 [N,H,W,cin]"""
        geom, w, b = self.layers[name]
        return conv_bias_relu(x, w, b, geom)

    def chain(self, block, names, x):
        for n in names:
            x = self.conv(f"{block}.{n}", x)
        return x

    def block(self, name, x):
        """one Mixed_* block on f32 [N,H,W,BLOCK_IN[name]]"""
        ch = lambda *names: self.chain(name, names, x)      # noqa: E731
        avg = "avg" if self.variant == "fid" else "avg_pad"
        if name in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
            outs = [ch("branch1x1"), ch("branch5x5_1", "branch5x5_2"), ch("branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"),
                    self.conv(name + ".branch_pool", ops.pool3x3(x, avg, 1))]
        elif name == "Mixed_6a":
            outs = [ch("branch3x3"), ch("branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"), ops.pool3x3(x, "max", 2)]
        elif name in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            outs = [ch("branch1x1"), ch("branch7x7_1", "branch7x7_2", "branch7x7_3"),
                    ch("branch7x7dbl_1", "branch7x7dbl_2", "branch7x7dbl_3", "branch7x7dbl_4", "branch7x7dbl_5"),
                    self.conv(name + ".branch_pool", ops.pool3x3(x, avg, 1))]
        elif name == "Mixed_7a":
            outs = [ch("branch3x3_1", "branch3x3_2"), ch("branch7x7x3_1", "branch7x7x3_2", "branch7x7x3_3", "branch7x7x3_4"),
                    ops.pool3x3(x, "max", 2)]
        elif name in ("Mixed_7b", "Mixed_7c"):
            b3, bd = ch("branch3x3_1"), ch("branch3x3dbl_1", "branch3x3dbl_2")
            pool = "max" if (name == "Mixed_7c" and self.variant == "fid") else avg                        # (7c: pytorch_fid's max pool)
            outs = [ch("branch1x1"), self.conv(name + ".branch3x3_2a", b3), self.conv(name + ".branch3x3_2b", b3),
                    self.conv(name + ".branch3x3dbl_3a", bd), self.conv(name + ".branch3x3dbl_3b", bd),
                    self.conv(name + ".branch_pool", ops.pool3x3(x, pool, 1))]
        else:
            raise KeyError(name)
        return torch.cat(outs, dim=3)

    def trunk(self, x8, with_mixed_6e=False):
        """f32 engine image [N,H,W,8] in [-1, 1] -> features f32 [N,2048]; ``with_mixed_6e``: (Mixed_6e's output [N,h,w,768], features)"""
        x = self.conv("Conv2d_1a_3x3", x8)
        x = self.conv("Conv2d_2a_3x3", x)
        x = self.conv("Conv2d_2b_3x3", x)
        x = ops.pool3x3(x, "max", 2)
        x = self.conv("Conv2d_3b_1x1", x)
        x = self.conv("Conv2d_4a_3x3", x)
        x = ops.pool3x3(x, "max", 2)
        mid = None
        for name in BLOCKS:
            x = self.block(name, x)
            if name == "Mixed_6e":
                mid = x
        N, H, W, Cc = x.shape
        y = torch.empty((N, Cc), dtype=torch.float32, device=x.device)
        L.call("xmc_global_avgpool", ops._p(x), ops._p(y), N, H * W, Cc, L.F32, L.F32, ops._st())
        return (mid, y) if with_mixed_6e else y


class InceptionFID(InceptionTrunk):
    """uint8 images [N,H,W,3] on the device -> pool3 features f32 [N,2048].  ``resize_to``: the side the front end resizes to (299, as
    pytorch_fid does; None: the images go in at their own size, which must be at least 75x75).  Frozen: nothing here is differentiable."""

    def __init__(self, weights=None, device="cuda", resize_to=299):
        super().__init__(load_inception_weights(weights), device, "fid")
        self.resize_to = resize_to
        self._weights, self._fc = weights, None

    def fc(self):
        """(geometry, weight) of the classifier as a 1x1 convolution: read from the weights file at the first call (`load_inception_fc`)"""
        if self._fc is None:
            w = load_inception_fc(self._weights).reshape(CLASSES, DIMS, 1, 1)
            self._fc = ConvGeom(DIMS, CLASSES, 1, 1, 0), torch.nn.Parameter(w.to(self.device).contiguous(), requires_grad=False)
        return self._fc

    @torch.no_grad()
    def logits(self, features):
        """pool3 rows f32 [N,2048] -> the 1008 logits f32 [N,1008] = features @ fc.weight.T, WITHOUT the bias (as the original Inception
        Score code and torch-fidelity take them): a 1x1 convolution on a 1x1 map, on the f32 implicit-GEMM path of the trunk"""
        f = ops._fid_arg(torch.as_tensor(features).to(self.device), "InceptionFID.logits", torch.float32, 2)
        if f.shape[1] != DIMS or f.shape[0] < 1:
            raise ValueError(f"InceptionFID.logits: feature rows [N,{DIMS}] expected, got {tuple(f.shape)}")
        geom, w = self.fc()
        y = _conv_fwd_raw(f.view(f.shape[0], 1, 1, DIMS), w, None, geom, L.ACT_NONE, torch.float32)
        return y.view(f.shape[0], -1)[:, :CLASSES]           # (1008 is a multiple of 8: the stored row has no padding column)

    @torch.no_grad()
    def __call__(self, u8):
        u8 = torch.as_tensor(u8)
        if u8.dim() != 4 or u8.shape[-1] != 3 or u8.dtype != torch.uint8:
            raise ValueError(f"InceptionFID: uint8 images [N,H,W,3] expected, got {u8.dtype} {tuple(u8.shape)}")
        u8 = u8.to(self.device)
        side = None if self.resize_to is None else (self.resize_to, self.resize_to)
        if min(side or u8.shape[1:3]) < 75:
            raise ValueError(f"InceptionFID: Inception-v3 needs at least 75x75 pixels, got {tuple(side or u8.shape[1:3])}")
        return self.trunk(ops.fid_resize_u8(u8, side))


def nchw_to_u8(images):
    """[B,3,H,W] images in [-1, 1] (what a generator returns and a loader yields) on the device -> uint8 [B,H,W,3] = trunc((x + 1) * 127.5):
    the bytes `utils.visual.to_uint8_hwc` puts into the PNGs, made from the f32 values whatever the precision mode"""
    x = images.detach().to(torch.float32).contiguous()
    ops._need_cuda(x)
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"nchw_to_u8: images [B,3,H,W] expected, got {tuple(x.shape)}")
    N, _, H, W = x.shape
    x8 = torch.empty((N, H, W, 8), dtype=torch.float32, device=x.device)
    L.call("xmc_nchw_to_nhwc8", ops._p(x), ops._p(x8), N, 3, H, W, L.F32, ops._st())
    y = torch.empty((N, H, W, 3), dtype=torch.uint8, device=x.device)
    L.call("xmc_image_to_u8", ops._p(x8), ops._p(y), N, H, W, L.F32, ops._st())
    return y


# ------------------------------------------------------------------------------------------ statistics
class FeatureStats:
    """running f64 sum and outer-product sum of feature rows, on the device (xmc_fid_moments)"""

    def __init__(self, dims=DIMS, device="cuda"):
        self.total = torch.zeros(dims, dtype=torch.float64, device=device)
        self.outer = torch.zeros((dims, dims), dtype=torch.float64, device=device)
        self.n = 0

    def update(self, features):
        ops.fid_moments(features, self.total, self.outer)
        self.n += int(features.shape[0])

    def finalize(self):
        """(mu [D], sigma [D,D]) as f64 numpy: the mean and np.cov(features, rowvar=False)"""
        if self.n < 2:
            raise ValueError(f"a covariance needs at least two samples, got {self.n}")
        mu = self.total.cpu().numpy() / self.n
        sigma = (self.outer.cpu().numpy() - self.n * np.outer(mu, mu)) / (self.n - 1)
        return mu, sigma

    def save(self, path):
        mu, sigma = self.finalize()
        save_stats(path, mu, sigma, self.n)
        return mu, sigma


def is_split_bounds(n, splits):
    """the parts of the Inception Score: [(s n // splits, (s + 1) n // splits)] -- consecutive rows in order of arrival, no shuffling"""
    n, splits = int(n), int(splits)
    if splits < 1 or n < splits:
        raise ValueError(f"the Inception Score over {splits} splits needs at least that many images, got {n}")
    return [(s * n // splits, (s + 1) * n // splits) for s in range(splits)]


def is_from_sums(H, P, n, splits):
    """(mean, std with ddof 0, the per-part scores) from `ops.inception_score_sums`' H [splits] and P [splits,C], in f64 on the host:
    part s scores exp(H_s / n_s - sum_y pbar log pbar), pbar = P_s / n_s (the mean KL divergence of p(y|x) from the part's marginal)"""
    H, P = np.asarray(H, np.float64), np.asarray(P, np.float64)
    scores = []
    for s, (lo, hi) in enumerate(is_split_bounds(n, splits)):
        pbar = P[s] / (hi - lo)
        pos = pbar > 0
        scores.append(np.exp(H[s] / (hi - lo) - float(np.sum(pbar[pos] * np.log(pbar[pos])))))
    scores = np.asarray(scores, np.float64)
    return float(scores.mean()), float(scores.std()), scores


class InceptionScore:
    """Inception Score (Salimans et al. 2016) of generated images: ``update(features)`` takes pool3 rows [B,2048] and keeps their 1008
    logits (`InceptionFID.logits`: no bias) in a `manifold.FeatureBank`; ``finalize()`` cuts them into ``splits`` consecutive parts and
    returns dict(inception_score, std, splits, n): mean and standard deviation (ddof 0) over the parts of exp(E_x KL(p(y|x) || p_s(y)))."""

    def __init__(self, extractor, splits=IS_SPLITS, device=None):
        from .manifold import FeatureBank
        self.extractor, self.splits = extractor, int(splits)
        if self.splits < 1:
            raise ValueError(f"InceptionScore: {splits} splits")
        extractor.fc()                                        # (a file without the classifier is refused here, not after the images)
        self.bank = FeatureBank(CLASSES, device or extractor.device)

    @property
    def n(self):
        return self.bank.n

    def update(self, features):
        self.bank.update(self.extractor.logits(features))

    def finalize(self):
        is_split_bounds(self.n, self.splits)
        H, P = ops.inception_score_sums(self.bank.rows(), self.splits)
        mean, std, _ = is_from_sums(H.cpu().numpy(), P.cpu().numpy(), self.n, self.splits)
        return dict(inception_score=mean, std=std, splits=self.splits, n=int(self.n))


def save_stats(path, mu, sigma, n=None):
    """pytorch_fid's statistics file: an .npz with ``mu`` and ``sigma`` (plus ``n``, the sample count, which pytorch_fid ignores)"""
    extra = {} if n is None else {"n": np.int64(n)}
    with open(path, "wb") as f:           # (a file object: np.savez appends nothing to the name)
        np.savez(f, mu=np.asarray(mu, np.float64), sigma=np.asarray(sigma, np.float64), **extra)


def load_stats(path, with_count=False):
    """(mu, sigma) of an .npz written by `save_stats` or by pytorch_fid; ``with_count``: (mu, sigma, n or None)"""
    with np.load(path) as z:
        if "mu" not in z.files or "sigma" not in z.files:
            raise ValueError(f"{path}: a statistics file holds 'mu' and 'sigma', this one holds {z.files}")
        mu, sigma = np.asarray(z["mu"], np.float64), np.asarray(z["sigma"], np.float64)
        n = int(z["n"]) if "n" in z.files else None
    if mu.ndim != 1 or sigma.shape != (mu.size, mu.size):
        raise ValueError(f"{path}: mu {mu.shape} / sigma {sigma.shape} are not a mean and its covariance")
    return (mu, sigma, n) if with_count else (mu, sigma)


def _psd_sqrt(s):
    """symmetric square root of a covariance from `eigh`, eigenvalues clamped at 0 -- and those within rounding of 0 (below dims * eps *
    the largest) set to 0: a null direction that rounding left at +1e-16 |s| would otherwise enter the root as 1e-8 |s|^(1/2)"""
    w, v = np.linalg.eigh(s)
    tol = max(float(w[-1]), 0.0) * w.size * np.finfo(np.float64).eps
    return (v * np.sqrt(np.where(w > tol, w, 0.0))) @ v.T


def frechet_distance(mu1, sigma1, mu2, sigma2):
    """|mu1 - mu2|^2 + tr s1 + tr s2 - 2 sum_i sqrt(lambda_i), lambda the eigenvalues of s1^(1/2) s2 s1^(1/2) (the spectrum of s1 s2, so
    the sum is tr sqrtm(s1 s2)).  The roots sqrt(lambda_i) are taken as the singular values of s2^(1/2) s1^(1/2) -- the same numbers,
    without the square root of a computed eigenvalue, which turns a rounding error of 1e-16 at a zero eigenvalue into 1e-8.  No scipy,
    no epsilon retry, and singular covariances (fewer samples than dimensions) need nothing special."""
    mu1, mu2 = np.asarray(mu1, np.float64), np.asarray(mu2, np.float64)
    s1, s2 = np.asarray(sigma1, np.float64), np.asarray(sigma2, np.float64)
    if mu1.shape != mu2.shape or s1.shape != s2.shape or s1.shape != (mu1.size, mu1.size):
        raise ValueError(f"frechet_distance: shapes {mu1.shape} {s1.shape} / {mu2.shape} {s2.shape}")
    roots = np.linalg.svd(_psd_sqrt(s2) @ _psd_sqrt(s1), compute_uv=False)
    diff = mu1 - mu2
    return float(diff @ diff + np.trace(s1) + np.trace(s2) - 2.0 * roots.sum())


def accumulate(acc, feature_batches):
    """``acc`` (a `FeatureStats`, a `manifold.FeatureBank`) after one update per batch of feature rows"""
    for feats in feature_batches:
        acc.update(feats)
    return acc


def fid_from_images(images_a, images_b, extractor, batch=100):
    """FID between two uint8 image sets [N,H,W,3] (tensors or arrays, host or device)"""
    sets = []
    for im in (images_a, images_b):
        im = torch.as_tensor(im)
        sets.append(accumulate(FeatureStats(DIMS, extractor.device), (extractor(im[i:i + batch]) for i in range(0, im.shape[0], batch))).finalize())
    return frechet_distance(*sets[0], *sets[1])


def list_images(directory):
    return sorted(os.path.join(directory, f) for f in os.listdir(directory) if f.lower().endswith(IMAGE_EXTENSIONS))


def _read_rgb(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def decoded_batches(files, batch=100):
    """the image files ``files``, ``batch`` at a time, as (their indices into ``files``, uint8 tensor [n,H,W,3]): decoded by PIL on up to 8
    host threads (no more than the process may run on); the files of a batch that share a size come together"""
    from concurrent.futures import ThreadPoolExecutor
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    with ThreadPoolExecutor(max(1, min(8, cores))) as pool:
        for i in range(0, len(files), batch):
            groups = {}
            for j, arr in enumerate(pool.map(_read_rgb, files[i:i + batch])):
                groups.setdefault(arr.shape, []).append((i + j, arr))
            for members in groups.values():
                yield [m[0] for m in members], torch.from_numpy(np.stack([m[1] for m in members]))


def features_of_dir(directory, extractor, batch=100):
    """the feature rows of the PNG / JPEG files of ``directory`` in sorted order, one tensor per group `decoded_batches` makes of them"""
    files = list_images(directory)
    if not files:
        raise ValueError(f"{directory} holds no image ({', '.join(IMAGE_EXTENSIONS)})")
    for _, u8 in decoded_batches(files, batch):
        yield extractor(u8)


def stats_of_dir(directory, extractor, batch=100):
    """`FeatureStats` of the image files of ``directory`` (`features_of_dir`)"""
    return accumulate(FeatureStats(DIMS, extractor.device), features_of_dir(directory, extractor, batch))


def stats_of(path, extractor, batch=100):
    """(mu, sigma) of an image directory or of an .npz statistics file"""
    if os.path.isdir(path):
        return stats_of_dir(path, extractor, batch).finalize()
    return load_stats(path)
