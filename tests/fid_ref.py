"""Plain-torch restatement of the FID Inception-v3 feature extractor, for the tests (a helper, not a test): written from the
architecture table of the FID variant (torchvision key names; BatchNorm eps 1e-3; 3x3 pools; the 5b-7b pool branches average over the
in-image pixels, 7c's is a max pool), on the CPU in f64 with F.conv2d / F.batch_norm / F.max_pool2d / F.avg_pool2d / F.interpolate,
NCHW.  `random_state_dict(seed)` makes weights in the upstream key layout that keep activations of order 1 through all 94 layers.
Shares no code with xmc_gan_amd/fid.py and reads nothing outside the repository."""
import torch
import torch.nn.functional as F

EPS = 1e-3


def _inc_a(m, cin, pf):
    return [(m + ".branch1x1", cin, 64, 1, 1, 0), (m + ".branch5x5_1", cin, 48, 1, 1, 0), (m + ".branch5x5_2", 48, 64, 5, 1, 2),
            (m + ".branch3x3dbl_1", cin, 64, 1, 1, 0), (m + ".branch3x3dbl_2", 64, 96, 3, 1, 1), (m + ".branch3x3dbl_3", 96, 96, 3, 1, 1),
            (m + ".branch_pool", cin, pf, 1, 1, 0)]


def _inc_c(m, c7):
    a, b = ((1, 7), (0, 3)), ((7, 1), (3, 0))
    return [(m + ".branch1x1", 768, 192, 1, 1, 0), (m + ".branch7x7_1", 768, c7, 1, 1, 0), (m + ".branch7x7_2", c7, c7, a[0], 1, a[1]),
            (m + ".branch7x7_3", c7, 192, b[0], 1, b[1]), (m + ".branch7x7dbl_1", 768, c7, 1, 1, 0),
            (m + ".branch7x7dbl_2", c7, c7, b[0], 1, b[1]), (m + ".branch7x7dbl_3", c7, c7, a[0], 1, a[1]),
            (m + ".branch7x7dbl_4", c7, c7, b[0], 1, b[1]), (m + ".branch7x7dbl_5", c7, 192, a[0], 1, a[1]),
            (m + ".branch_pool", 768, 192, 1, 1, 0)]


def _inc_e(m, cin):
    a, b = ((1, 3), (0, 1)), ((3, 1), (1, 0))
    return [(m + ".branch1x1", cin, 320, 1, 1, 0), (m + ".branch3x3_1", cin, 384, 1, 1, 0), (m + ".branch3x3_2a", 384, 384, a[0], 1, a[1]),
            (m + ".branch3x3_2b", 384, 384, b[0], 1, b[1]), (m + ".branch3x3dbl_1", cin, 448, 1, 1, 0),
            (m + ".branch3x3dbl_2", 448, 384, 3, 1, 1), (m + ".branch3x3dbl_3a", 384, 384, a[0], 1, a[1]),
            (m + ".branch3x3dbl_3b", 384, 384, b[0], 1, b[1]), (m + ".branch_pool", cin, 192, 1, 1, 0)]


def layer_table():
    """[(name, cin, cout, kernel, stride, padding)]; kernel / padding an int or a (height, width) pair"""
    t = [("Conv2d_1a_3x3", 3, 32, 3, 2, 0), ("Conv2d_2a_3x3", 32, 32, 3, 1, 0), ("Conv2d_2b_3x3", 32, 64, 3, 1, 1),
         ("Conv2d_3b_1x1", 64, 80, 1, 1, 0), ("Conv2d_4a_3x3", 80, 192, 3, 1, 0)]
    t += _inc_a("Mixed_5b", 192, 32) + _inc_a("Mixed_5c", 256, 64) + _inc_a("Mixed_5d", 288, 64)
    t += [("Mixed_6a.branch3x3", 288, 384, 3, 2, 0), ("Mixed_6a.branch3x3dbl_1", 288, 64, 1, 1, 0),
          ("Mixed_6a.branch3x3dbl_2", 64, 96, 3, 1, 1), ("Mixed_6a.branch3x3dbl_3", 96, 96, 3, 2, 0)]
    t += _inc_c("Mixed_6b", 128) + _inc_c("Mixed_6c", 160) + _inc_c("Mixed_6d", 160) + _inc_c("Mixed_6e", 192)
    t += [("Mixed_7a.branch3x3_1", 768, 192, 1, 1, 0), ("Mixed_7a.branch3x3_2", 192, 320, 3, 2, 0),
          ("Mixed_7a.branch7x7x3_1", 768, 192, 1, 1, 0), ("Mixed_7a.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3)),
          ("Mixed_7a.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0)), ("Mixed_7a.branch7x7x3_4", 192, 192, 3, 2, 0)]
    t += _inc_e("Mixed_7b", 1280) + _inc_e("Mixed_7c", 2048)
    return t


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def random_state_dict(seed, only=None):
    """f32 state dict in the upstream key layout: conv weights ~ N(0, 2 / fan_in), BatchNorm gamma 1 +- 0.1, beta / running mean
    N(0, 0.1), running variance in [0.8, 1.2], plus the ``fc.*`` and ``num_batches_tracked`` entries a loader has to ignore.
    ``only``: a name prefix (one block's layers alone, for the block tests)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, cin, cout, k, _, _ in layer_table():
        if only is not None and not name.startswith(only):
            continue
        kh, kw = _pair(k)
        sd[name + ".conv.weight"] = torch.randn(cout, cin, kh, kw, generator=g) * (2.0 / (cin * kh * kw)) ** 0.5
        sd[name + ".bn.weight"] = 1.0 + 0.1 * torch.randn(cout, generator=g)
        sd[name + ".bn.bias"] = 0.1 * torch.randn(cout, generator=g)
        sd[name + ".bn.running_mean"] = 0.1 * torch.randn(cout, generator=g)
        sd[name + ".bn.running_var"] = 0.8 + 0.4 * torch.rand(cout, generator=g)
        sd[name + ".bn.num_batches_tracked"] = torch.tensor(0)
    if only is None:
        sd["fc.weight"], sd["fc.bias"] = torch.zeros(1008, 2048), torch.zeros(1008)
    return sd


class Reference:
    """the extractor on the CPU in f64, NCHW"""

    def __init__(self, sd):
        self.sd = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
        self.geo = {name: (k, s, p) for name, _, _, k, s, p in layer_table()}

    def conv(self, name, x):
        k, s, p = self.geo[name]
        sd = self.sd
        y = F.conv2d(x, sd[name + ".conv.weight"], None, stride=s, padding=_pair(p))
        y = F.batch_norm(y, sd[name + ".bn.running_mean"], sd[name + ".bn.running_var"], sd[name + ".bn.weight"], sd[name + ".bn.bias"],
                         training=False, eps=EPS)
        return F.relu(y)

    def seq(self, m, names, x):
        for n in names:
            x = self.conv(m + "." + n, x)
        return x

    @staticmethod
    def avg(x):
        return F.avg_pool2d(x, 3, stride=1, padding=1, count_include_pad=False)

    def block(self, m, x):
        if m[:7] == "Mixed_5":
            return torch.cat([self.conv(m + ".branch1x1", x), self.seq(m, ["branch5x5_1", "branch5x5_2"], x),
                              self.seq(m, ["branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"], x),
                              self.conv(m + ".branch_pool", self.avg(x))], 1)
        if m == "Mixed_6a":
            return torch.cat([self.conv(m + ".branch3x3", x), self.seq(m, ["branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"], x),
                              F.max_pool2d(x, 3, stride=2)], 1)
        if m[:7] == "Mixed_6":
            return torch.cat([self.conv(m + ".branch1x1", x), self.seq(m, ["branch7x7_1", "branch7x7_2", "branch7x7_3"], x),
                              self.seq(m, ["branch7x7dbl_%d" % i for i in range(1, 6)], x), self.conv(m + ".branch_pool", self.avg(x))], 1)
        if m == "Mixed_7a":
            return torch.cat([self.seq(m, ["branch3x3_1", "branch3x3_2"], x),
                              self.seq(m, ["branch7x7x3_%d" % i for i in range(1, 5)], x), F.max_pool2d(x, 3, stride=2)], 1)
        assert m in ("Mixed_7b", "Mixed_7c")
        b3 = self.conv(m + ".branch3x3_1", x)
        b3 = torch.cat([self.conv(m + ".branch3x3_2a", b3), self.conv(m + ".branch3x3_2b", b3)], 1)
        bd = self.seq(m, ["branch3x3dbl_1", "branch3x3dbl_2"], x)
        bd = torch.cat([self.conv(m + ".branch3x3dbl_3a", bd), self.conv(m + ".branch3x3dbl_3b", bd)], 1)
        pooled = self.avg(x) if m == "Mixed_7b" else F.max_pool2d(x, 3, stride=1, padding=1)
        return torch.cat([self.conv(m + ".branch1x1", x), b3, bd, self.conv(m + ".branch_pool", pooled)], 1)

    @staticmethod
    def front_end(u8_nhwc, resize_to=299):
        """uint8 [N,H,W,3] -> f64 [N,3,S,S] in [-1, 1]"""
        x = torch.as_tensor(u8_nhwc).permute(0, 3, 1, 2).double() / 255.0
        if resize_to is not None:
            x = F.interpolate(x, size=(resize_to, resize_to), mode="bilinear", align_corners=False)
        return 2.0 * x - 1.0

    def trunk(self, x):
        for n in ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"):
            x = self.conv(n, x)
        x = F.max_pool2d(x, 3, stride=2)
        x = self.conv("Conv2d_4a_3x3", self.conv("Conv2d_3b_1x1", x))
        x = F.max_pool2d(x, 3, stride=2)
        for m in ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7a", "Mixed_7b",
                  "Mixed_7c"):
            x = self.block(m, x)
        return x.mean((2, 3))

    def features(self, u8_nhwc, resize_to=299):
        with torch.no_grad():
            return self.trunk(self.front_end(u8_nhwc, resize_to))


def trunk_f32_on(sd, device):
    """the same forward as `Reference.trunk` in f32 on `device` (tests/bench_fid.py: plain torch on the card, beside the native path)"""
    ref = Reference(sd)
    ref.sd = {k: v.to(device, torch.float32) for k, v in ref.sd.items()}
    return ref
