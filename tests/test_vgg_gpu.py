"""TRAIN.ENCODER_LOSS.VGG on the GPU: csrc/vgg.hip against the f64 restatement (tests/vgg_ref.py), the frozen VGG-19 at full width against
yardsticks measured inside the test, the term through `VGGContrast` + `img_loss`, and the generator step that carries it.

The bars of the network tests are not numbers fixed in advance.  Each test measures, against the f64 restatement,
  * the engine's error, and
  * a yardstick's error on the same inputs: in fp32 mode the same forward / backward in plain torch f32 on the CPU, in the 16-bit modes
    `vgg_ref.emulate(fmt)` (f32 arithmetic, activations and their gradients rounded to the format after every layer),
and asks for engine <= 8 x yardstick (fp32) or 4 x yardstick (bf16 / f16).  The factors cover another accumulation order over K up to 4608 and
16 layers; they do not cover another algorithm.  Rows: max abs error / rms of the reference.  Image gradient: rms of the difference / rms of the reference (an arg-max that flips
on a rounding-level near-tie moves single pixels and must not decide the test).

The random weights lie on values that f32, bf16 and IEEE half all hold exactly (vgg_ref.random_weights), as the images do: the 16-bit modes
store their convolution weights in the 16-bit format, and that one rounding -- the format's precision, coherent over the pixels a row
averages -- is not in the yardstick; with weights off the grid the 64x64 rows measured x6.5 (bf16) / x7.4 (f16) of the yardstick for that
reason alone (figures and the check of the reason: vgg_ref.random_weights).

Measured on an MI355X, engine / yardstick (ratio), weights on the grid:
  all of features, 32x32     fp32  rows 5.8e-6 / 1.5e-6 (x3.9)    image gradient 2.1e-6 / 6.0e-7 (x3.6)
                             bf16  rows 1.63e-2 / 1.53e-2 (x1.07)  image gradient 2.54e-1 / 2.35e-1 (x1.08)
                             f16   rows 2.54e-3 / 1.90e-3 (x1.34)  image gradient 8.01e-2 / 6.10e-2 (x1.31)
  conv1_1 .. pool2, 64x64    fp32  rows 2.8e-7 / 2.6e-7 (x1.1)    image gradient 6.2e-7 / 2.8e-7 (x2.2)
                             bf16  rows 6.25e-4 / 6.81e-4 (x0.92)  image gradient 1.279e-1 / 1.280e-1 (x1.00)
                             f16   rows 9.40e-5 / 8.91e-5 (x1.05)  image gradient 3.82e-2 / 4.26e-2 (x0.90)
  VGGContrast + img_loss     image gradient: fp32 x3.7 / x3.8 (identity labels / B_GLOBAL), bf16 x1.03 / x1.02, f16 x1.10 / x1.10; the loss
                             (f64 value 2.7717 / 1.7325): the pairs and the two floors of its bar are in that test's docstring
(8 significant bits through 16 random layers and five arg-max stages cost a quarter of the image gradient in rms, in the yardstick as in the
engine: that is bf16, not a kernel.)  The same table: profiles/README.md, "VGG loss".
"""
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vgg_ref as R  # noqa: E402
import xmc_ref as X  # noqa: E402
from parity_util import DEV, GradTap, build_product, setup_cfg  # noqa: E402
from xmc_gan_amd import lib as L  # noqa: E402
from xmc_gan_amd import ops, prof  # noqa: E402
from xmc_gan_amd.vgg import VGG19Features, VGGContrast  # noqa: E402

MODES = ["fp32", "bf16", "f16"]
FMT = {"fp32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
FACTOR = {"fp32": 8.0, "bf16": 4.0, "f16": 4.0}
F32_EPS = 2.0 ** -24
SECOND = 1 + 2.0 ** -7          # the second-order terms of the prep bounds (a rounding of a rounded value): at most u times the bound


@pytest.fixture(autouse=True)
def _restore_precision():
    yield
    ops.set_precision("bf16")


@functools.lru_cache(maxsize=None)
def _weights():
    return R.random_weights(11)


@pytest.fixture(scope="module")
def weights_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("vgg") / "vgg19.pth")
    R.write_weights_file(path, weights=_weights())
    return path


def _lattice(shape, gen, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


def _image(N, H, W, seed):
    """[N,3,H,W] f64 in [-1, 1] on the grid of 1/128: the same values in f32, bf16 and IEEE half"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-128, 129, (N, 3, H, W), generator=g).double() / 128


# ------------------------------------------------------------------------------------------ vgg_prep
@pytest.mark.parametrize("shape", [(2, 4, 4), (2, 6, 2), (3, 40, 28)], ids=lambda s: "x".join(map(str, s)))   # (the last: four workgroups)
@pytest.mark.parametrize("mode", MODES)
def test_vgg_prep_forward_and_backward(mode, shape):
    """against f64, up to one rounding of the output dtype in front of which stands the f32 arithmetic, bounded term by term (u32 = 2^-24):
    t = fma(x, 1/2, 1/2 - mean) is one rounding of a value of at most 1.02 plus the constant's own rounding (|1/2 - mean| < 0.1):
    |dt| <= 1.1 u32, which the division carries into the result as 1.1 u32 / std_c -- an ABSOLUTE term, the one that matters where t cancels to
    near zero; the division adds std's rounding to f32 and its own, 3 u32 |ref| with a unit to spare for a divide that is good to one ulp
    rather than half.  So e32 = u32 (1.1 / std_c + 3 |ref|), and |y - ref| <= e32 in fp32 mode (the division's rounding IS the output's),
    u |ref| + e32 in the 16-bit modes (u the format's unit roundoff).  Backward: one product with a constant rounded to f32,
    (u + 2 u32) |ref| (fp32: 2 u32 |ref|).  The padding channels hold noise on the way in and exact zeros on the way out, both ways.
    The last shape takes several workgroups; the grid-stride loop has a test of its own below."""
    ops.set_precision(mode)
    dt, (N, H, W) = FMT[mode], shape
    u = 0.0 if mode == "fp32" else torch.finfo(dt).eps / 2
    g = torch.Generator().manual_seed(N * 100 + H)
    x = _image(N, H, W, seed=H * 7 + W)
    x_h = R.to_engine(x, dt)
    x_h[..., 3:] = (torch.randn(N, H, W, 5, generator=g) * 50).to(dt)
    x_h = x_h.to(DEV).requires_grad_()
    y = ops.vgg_prep(x_h)
    assert y.dtype == dt and y.shape == x_h.shape and (y[..., 3:] == 0).all()
    ref = R.prep(x)
    e32 = F32_EPS * (1.1 / torch.tensor(R.STD, dtype=torch.float64).view(1, 3, 1, 1) + 3 * ref.abs())
    err = (R.from_engine(y) - ref).abs()
    assert (err <= SECOND * (u * ref.abs() + e32)).all(), (err / (u * ref.abs() + e32)).max()
    dy = (torch.randn(N, 3, H, W, generator=g, dtype=torch.float64)).to(dt).double()
    dy_h = R.to_engine(dy, dt)
    dy_h[..., 3:] = (torch.randn(N, H, W, 5, generator=g) * 50).to(dt)
    (dx,) = torch.autograd.grad(y, x_h, dy_h.to(DEV))
    assert dx.dtype == dt and (dx[..., 3:] == 0).all()
    ref = R.prep_bwd(dy)
    err = (R.from_engine(dx) - ref).abs()
    assert (err <= SECOND * (u + 2 * F32_EPS) * ref.abs()).all(), (err / ((u + 2 * F32_EPS) * ref.abs()).clamp_min(1e-30)).max()
    print(f"\n[vgg_prep {mode} {shape}] forward and backward within one rounding of {dt}")


# ------------------------------------------------------------------------------------------ relu_maxpool2
@pytest.mark.parametrize("hw", [(2, 2), (4, 6), (6, 4), (16, 12)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", MODES)
def test_relu_maxpool2_is_bit_equal_on_lattices_full_of_ties(mode, hw):
    """integer values in [-2, 2] (exact in every dtype, ties certain), with an all-negative window, a window whose maximum is exactly 0 and a
    four-way positive tie planted; C = 72 is no multiple of 64, (16, 12) with N = 3 takes several workgroups.  Forward and backward bit-equal to
    the restatement, whose backward rule tests/test_vgg_cpu.py checks against torch.autograd."""
    ops.set_precision(mode)
    dt, (H, W) = FMT[mode], hw
    N = 3 if hw == (16, 12) else 2
    for C in (8, 24, 72):
        g = torch.Generator().manual_seed(H * 1000 + W * 10 + C)
        z = _lattice((N, C, H, W), g, -2, 2)
        z[0, 0, :2, :2] = -1.0
        z[0, 1, :2, :2] = torch.tensor([[-2.0, 0.0], [0.0, -1.0]], dtype=torch.float64)
        z[0, 2, :2, :2] = 2.0
        z[1, C - 1, H - 2:, W - 2:] = torch.tensor([[1.0, 2.0], [2.0, 2.0]], dtype=torch.float64)      # the tie starts at the second position
        dp = _lattice((N, C, H // 2, W // 2), g, 1, 4)
        z_h = z.permute(0, 2, 3, 1).contiguous().to(dt).to(DEV).requires_grad_()
        p = ops.relu_maxpool2(z_h)
        assert p.dtype == dt and tuple(p.shape) == (N, H // 2, W // 2, C)
        (dz,) = torch.autograd.grad(p, z_h, dp.permute(0, 2, 3, 1).contiguous().to(dt).to(DEV))
        assert torch.equal(R.from_engine(p, C), R.relu_maxpool2(z)), (mode, hw, C)
        want = R.relu_maxpool2_bwd(z, dp)
        assert torch.equal(R.from_engine(dz, C), want), (mode, hw, C)
        assert want[0, 2, 0, 0] == dp[0, 2, 0, 0] and want[0, :2, :2, :2].abs().sum() == 0 and want[1, C - 1, H - 2, W - 1] == dp[1, C - 1, -1, -1]


def test_grid_stride_loops_on_maps_of_more_than_4096_workgroups():
    """the three kernels cap their grid at 4096 workgroups and stride beyond it: more than 256 * 4096 pool units (N = 2, 512x512, C = 72:
    1.18 M units, 75 MB in bf16) and more than 1024 * 4096 prep units (one image of 2048x2112 pixels: 4.3 M, 69 MB).  bf16; the pool bit-equal
    on the lattice to the restatement run in torch on the device, prep within the bound of test_vgg_prep_forward_and_backward."""
    ops.set_precision("bf16")
    dt, g = torch.bfloat16, torch.Generator(device=DEV).manual_seed(3)
    N, H, W, C = 2, 512, 512, 72
    assert N * (H // 2) * (W // 2) * (C // 8) > 256 * 4096
    z = torch.randint(-2, 3, (N, C, H, W), generator=g, device=DEV).float()
    dp = torch.randint(1, 5, (N, C, H // 2, W // 2), generator=g, device=DEV).float()
    z_h = z.permute(0, 2, 3, 1).contiguous().to(dt).requires_grad_()
    p = ops.relu_maxpool2(z_h)
    (dz,) = torch.autograd.grad(p, z_h, dp.permute(0, 2, 3, 1).contiguous().to(dt))
    assert torch.equal(p.float().permute(0, 3, 1, 2), R.relu_maxpool2(z))
    assert torch.equal(dz.float().permute(0, 3, 1, 2), R.relu_maxpool2_bwd(z, dp))
    del z, dp, z_h, p, dz
    H, W = 2048, 2112
    assert H * W > 1024 * 4096
    x = torch.randint(-128, 129, (1, 3, H, W), generator=g, device=DEV).double() / 128
    dy = torch.randn(1, 3, H, W, generator=g, device=DEV).to(dt).double()
    x_h = torch.zeros(1, H, W, 8, dtype=dt, device=DEV)
    x_h[..., :3] = x.permute(0, 2, 3, 1).to(dt)
    dy_h = torch.ones(1, H, W, 8, dtype=dt, device=DEV)
    dy_h[..., :3] = dy.permute(0, 2, 3, 1).to(dt)
    x_h.requires_grad_()
    y = ops.vgg_prep(x_h)
    (dx,) = torch.autograd.grad(y, x_h, dy_h)
    assert (y[..., 3:] == 0).all() and (dx[..., 3:] == 0).all()
    u, std = torch.finfo(dt).eps / 2, torch.tensor(R.STD, dtype=torch.float64, device=DEV).view(1, 3, 1, 1)
    mean = torch.tensor(R.MEAN, dtype=torch.float64, device=DEV).view(1, 3, 1, 1)
    ref = ((x + 1) / 2 - mean) / std
    assert ((y[..., :3].double().permute(0, 3, 1, 2) - ref).abs() <= SECOND * (u * ref.abs() + F32_EPS * (1.1 / std + 3 * ref.abs()))).all()
    ref = dy * (0.5 / std)
    assert ((dx[..., :3].double().permute(0, 3, 1, 2) - ref).abs() <= SECOND * (u + 2 * F32_EPS) * ref.abs()).all()


def test_relu_maxpool2_refuses_odd_heights_and_channel_counts_that_are_no_multiple_of_8():
    ops.set_precision("bf16")
    for shape in ((1, 3, 4, 8), (1, 4, 3, 8), (1, 2, 2, 12)):
        with pytest.raises(L.XmcHipError, match="XMC_ESHAPE"):
            ops.relu_maxpool2(torch.zeros(shape, dtype=torch.bfloat16, device=DEV))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ the network at full width
CASES = {"all of features, 32x32": (3, 32, 5), "conv1_1 .. pool2, 64x64": (2, 64, 2)}      # N, side, stages


def _rows_and_grad(fn, x, r):
    x = x.clone().requires_grad_()
    rows = fn(x)
    (gx,) = torch.autograd.grad((rows * r.to(rows.dtype)).sum(), x)
    return rows.detach().double(), gx.detach().double()


@functools.lru_cache(maxsize=None)
def _reference(case):
    """(image, r, f64 rows, f64 image gradient of sum(rows * r)): computed once, shared by the three modes"""
    N, S, stages = CASES[case]
    x = _image(N, S, S, seed=S + stages)
    r = torch.randn(N, (512, 128)[stages == 2], generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    return (x, r) + _rows_and_grad(lambda t: R.forward(t, _weights(), stages), x, r)


@functools.lru_cache(maxsize=None)
def _yardstick(case, mode):
    x, r, _, _ = _reference(case)
    stages = CASES[case][2]
    fn = (lambda t: R.forward(t, _weights(), stages, dtype=torch.float32)) if mode == "fp32" else \
        (lambda t: R.emulate(FMT[mode])(t, _weights(), stages))
    return _rows_and_grad(fn, x.float(), r)


def _row_err(a, ref):
    return ((a - ref).abs().max() / ref.pow(2).mean().sqrt()).item()


def _rms_err(a, ref):
    return ((a - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("mode", MODES)
def test_network_against_the_calibrated_yardstick(mode, case, weights_file):
    """(module docstring for the bars.)  The 64x64 case stops after pool2: that is where the large-map 3x3 kernels are dispatched."""
    ops.set_precision(mode)
    N, S, stages = CASES[case]
    x, r, rows_ref, gx_ref = _reference(case)
    rows_y, gx_y = _yardstick(case, mode)
    net = VGG19Features(weights_file, DEV)
    x_h = R.to_engine(x, FMT[mode]).to(DEV).requires_grad_()
    rows = net(x_h, stages)
    assert rows.dtype == torch.float32 and tuple(rows.shape) == tuple(rows_ref.shape)
    (gx,) = torch.autograd.grad((rows * r.float().to(DEV)).sum(), x_h)
    assert gx.dtype == FMT[mode] and (gx[..., 3:] == 0).all()
    assert all(p.grad is None for p in net.parameters())
    e_rows, y_rows = _row_err(rows.cpu().double(), rows_ref), _row_err(rows_y, rows_ref)
    e_gx, y_gx = _rms_err(R.from_engine(gx), gx_ref), _rms_err(gx_y, gx_ref)
    print(f"\n[vgg network {mode}, {case}] rows: engine {e_rows:.3e} yardstick {y_rows:.3e} (x{e_rows / y_rows:.2f}); "
          f"image gradient: engine {e_gx:.3e} yardstick {y_gx:.3e} (x{e_gx / y_gx:.2f}); allowed x{FACTOR[mode]:g}")
    assert e_rows <= FACTOR[mode] * y_rows and e_gx <= FACTOR[mode] * y_gx


# ------------------------------------------------------------------------------------------ VGGContrast + img_loss
@functools.lru_cache(maxsize=None)
def _contrast_reference(b_global, dtype=torch.float64, fmt=None, smooth=0.0):
    """the restatement composed with the oracle's img_loss at N = 4, 32 px: (real image, generated image, labels, loss, d loss / d generated
    image, real rows, generated rows, d loss / d rows)"""
    real, fake = _image(4, 32, 32, seed=21), _image(4, 32, 32, seed=22)
    sent = torch.randn(4, 16, generator=torch.Generator().manual_seed(23))
    sent[1] = sent[0] + 0.05 * sent[1]                               # B_GLOBAL: captions 0 and 1 are global positives of each other
    labels = X.make_labels(4, sent, b_global, smooth_global=smooth)
    net = lambda t: R.forward(t, _weights(), 5, dtype=dtype, fmt=fmt)      # noqa: E731
    fk = fake.to(dtype).requires_grad_()
    a = net(real.to(dtype)).detach().requires_grad_()
    b = net(fk)
    loss = X.contrastive_loss(a, b, labels.to(dtype), b_global, smooth_global=smooth)
    gx, ga, gb = torch.autograd.grad(loss, (fk, a, b))
    return real, fake, sent, labels, loss.detach().double(), gx.double(), a.detach().double(), b.detach().double(), ga.double(), gb.double()


@pytest.mark.parametrize("b_global", [False, True], ids=["identity-labels", "B_GLOBAL"])
@pytest.mark.parametrize("mode", MODES)
def test_contrast_rows_through_img_loss(mode, b_global, weights_file):
    """loss and d loss / d generated image against the restatement composed with the oracle's img_loss, under the calibrated bars of the module
    docstring: engine error <= FACTOR x the yardstick's error, for the rows, the image gradient and the loss.

    The loss is ONE number, and its yardstick error has two floors, both of the size of the errors measured, neither above them by more
    than a small factor:
      * expected: |d loss / d rows|_2 x rms(yardstick row error), what the yardstick's row errors give the loss on average at first order
        (from the f64 reference).  It IS the yardstick's loss error where luck plays no part -- bf16: 2.00e-5 / 9.7e-6 beside the measured
        2.21e-5 / 1.10e-5 (identity labels / B_GLOBAL) -- and stands in where the single measured number came out small by chance:
        IEEE half, B_GLOBAL: yardstick 2.49e-7 where its rows promise 1.20e-6 (identity labels: 1.37e-6 beside 2.47e-6).  There the
        engine's 9.64e-7 is inside 4 x 2.49e-7 = 9.95e-7 by 3 %: a pass that the next change of a summation order would turn over.
      * one rounding of the result: 2^-24 |loss|.  img_loss returns an f32 number.  In fp32 mode the row errors promise 2e-9 / 1e-9 and
        what is measured is the rounding of the f32 result: yardstick 6.2e-8 / 1.03e-8 on the machine of the measurement (1.76e-7 / 1.03e-8
        on another: the CPU's own summation order), the engine the same two f32 numbers, bit for bit.  One f32 ulp of 1.73 is 1.2e-7, more
        than 8 x 1.03e-8: without the floor the B_GLOBAL case tests whether two roundings fell the same way.
    Without either floor all six cases pass as measured (engine / yardstick: fp32 6.2e-8 / 6.2e-8 and 1.03e-8 / 1.03e-8, bf16 1.83e-5 /
    2.19e-5 and 1.10e-5 / 1.10e-5, IEEE half 1.85e-6 / 1.37e-6 and 9.64e-7 / 2.49e-7); the floors are there for the two named cases."""
    import xmc_gan.train_gan as tg
    ops.set_precision(mode)
    cfg, _ = setup_cfg("df_gan_damsm.yml", **{"TRAIN.ENCODER_LOSS.B_GLOBAL": b_global})
    assert cfg.TRAIN.SMOOTH.GLOBAL == 0.0          # (`_contrast_reference`'s smooth: every global positive weighs 1 / num_pos)
    real, fake, sent, labels, loss_ref, gx_ref, a_ref, b_ref, ga_ref, gb_ref = _contrast_reference(b_global)
    y = _contrast_reference(b_global, torch.float32, None if mode == "fp32" else FMT[mode])
    loss_y, gx_y, a_y, b_y = y[4], y[5], y[6], y[7]
    dev_labels = tg.make_labels(4, sent.to(DEV), b_global)
    assert torch.equal(dev_labels.cpu(), labels)
    contrast = VGGContrast(VGG19Features(weights_file, DEV))
    fake_h = R.to_engine(fake, FMT[mode]).to(DEV).requires_grad_()
    real_rows, fake_rows = contrast.rows(R.to_engine(real, FMT[mode]).to(DEV), fake_h)
    assert not real_rows.requires_grad and fake_rows.requires_grad and real_rows.dtype == fake_rows.dtype == torch.float32
    loss = tg.img_loss(real_imgs=real_rows, fake_imgs=fake_rows, labels=dev_labels, b_global=b_global)
    (gx,) = torch.autograd.grad(loss, fake_h)
    rows_ref, rows_y, rows_e = torch.cat((a_ref, b_ref)), torch.cat((a_y, b_y)), torch.cat((real_rows, fake_rows)).detach().cpu().double()
    e_rows, y_rows = _row_err(rows_e, rows_ref), _row_err(rows_y, rows_ref)
    expected = torch.cat((ga_ref, gb_ref)).norm().item() * (rows_y - rows_ref).pow(2).mean().sqrt().item()
    y_loss_raw = abs(loss_y.item() - loss_ref.item())
    e_loss, y_loss = abs(loss.item() - loss_ref.item()), max(y_loss_raw, expected, F32_EPS * abs(loss_ref.item()))
    e_gx, y_gx = _rms_err(R.from_engine(gx), gx_ref), _rms_err(gx_y, gx_ref)
    print(f"\n[vgg contrast {mode}, {'B_GLOBAL' if b_global else 'identity labels'}] loss {loss.item():.6f} (f64 {loss_ref.item():.6f}): engine "
          f"{e_loss:.3e}, yardstick {y_loss_raw:.3e} (expected from its rows {expected:.3e}, one f32 rounding {F32_EPS * abs(loss_ref.item()):.3e}); rows: engine {e_rows:.3e} yardstick "
          f"{y_rows:.3e}; image gradient: engine {e_gx:.3e} yardstick {y_gx:.3e} (x{e_gx / y_gx:.2f}); allowed x{FACTOR[mode]:g}")
    assert e_rows <= FACTOR[mode] * y_rows and e_loss <= FACTOR[mode] * y_loss and e_gx <= FACTOR[mode] * y_gx


# ------------------------------------------------------------------------------------------ the iteration
class _Calls:
    """the library calls that go through lib.call, in order"""

    def __init__(self, monkeypatch):
        self.names = []
        orig = L.call

        def call(name, *a):
            self.names.append(name)
            return orig(name, *a)
        monkeypatch.setattr(L, "call", call)

    def vgg(self):
        return [n for n in self.names if n.startswith(("xmc_vgg", "xmc_relu_maxpool2"))]


def _iteration(vgg_on, opts, lr=None, steps=1, graph=False):
    """``steps`` iterations at 64 px, batch 4, NCH 8 on fresh modules from the oracle's synthetic parameters, eagerly or through
    `GraphedIteration` (two eager warm-ups, then capture and replay): (the last iteration's losses, the generator gradients of each step)"""
    import xmc_gan.train_gan as tg
    from xmc_gan_amd.graph import GraphedIteration
    from xmc_gan_amd.optim import HipAdam
    cfg, h = setup_cfg("df_gan_damsm.yml", **{"TRAIN.NCH": 8, "TRAIN.ENCODER_LOSS.VGG": vgg_on})
    assert cfg.IMG.SIZE == 64 and cfg.TRAIN.N_CRITIC == 1
    netG, netD, optG, optD = build_product(h, X.synth_params(X.gen_shapes(h), 5), X.synth_params(X.netd_shapes(h), 6), 1e-3)
    if lr is not None:
        optG = HipAdam(netG.parameters(), lr=lr, betas=h.g_betas, eps=1e-3)
        optD = HipAdam(netD.parameters(), lr=lr, betas=h.d_betas, eps=1e-3)
    tap = GradTap(optG, netG.named_parameters()) if not graph else None      # (the tap reads the gradients back: not inside a capture)
    b = X.synth_batch(h, 4, seed=500, words_len=cfg.TEXT.MAX_LENGTH)
    batch = [b[k].to(DEV) for k in ("imgs", "sent_embs", "words_embs", "mask", "noise")]
    state = {}
    run = GraphedIteration(lambda *a: tg.gan_iteration(netG, netD, optG, optD, *a, opts), batch, n_critic=1, warmup=2) if graph else None
    try:
        for _ in range(steps):
            out = dict(run(*batch)) if graph else tg.gan_iteration(netG, netD, optG, optD, *batch, state, opts)
        torch.cuda.synchronize()
        replayed = graph and bool(run.seqs)
        out = {k: v.detach().float().cpu().clone() for k, v in out.items()}
    finally:
        if run is not None:
            run.close()
    return out, (tap.records if tap is not None else None), batch, replayed


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_iteration_carries_the_term(mode, weights_file):
    """`gan_iteration` with E.VGG on finishes with a finite vgg_loss, and that number is `VGGContrast` + `img_loss` on the iteration's own real
    and generated images (the f32 image the iteration returns holds the engine image's values exactly).  Both sides run the same kernels on the
    same bytes; what is free is the order of f32 sums inside the contrastive kernels: 1e-5 relative, the bar the entry-point tests use for an
    iteration launched two ways.  With --vgg_smooth 0 the generator's gradients are those of the iteration with E.VGG off, to rounding: the
    term's branch hands zeros to the generated image, so the two differ by at most how one gradient tensor is summed and stored -- one rounding
    of the activation dtype, per tensor 1e-5 (fp32, with the weight gradients' f32 atomics) / 2^-8 (bf16) in relative L2."""
    import xmc_gan.train_gan as tg
    ops.set_precision(mode)
    contrast = VGGContrast(VGG19Features(weights_file, DEV).warm())
    out, grads_on, batch, _ = _iteration(True, tg.StepOptions(vgg=contrast))
    assert torch.isfinite(out["vgg_loss"]) and out["vgg_loss"] > 0 and torch.isfinite(out["errG"])
    real_rows, fake_rows = contrast.rows(ops.to_nhwc8(batch[0]), ops.to_nhwc8(out["fake"].to(DEV)))
    want = tg.img_loss(real_imgs=real_rows, fake_imgs=fake_rows.detach(), labels=tg.make_labels(4, batch[1].float(), False), b_global=False).item()
    print(f"\n[vgg iteration {mode}] vgg_loss {out['vgg_loss'].item():.7f}, VGGContrast on the iteration's images {want:.7f}")
    assert abs(out["vgg_loss"].item() - want) <= 1e-5 * abs(want) + 1e-6
    out0, grads_zero, _, _ = _iteration(True, tg.StepOptions(vgg=contrast, vgg_smooth=0.0))
    out_off, grads_off, _, _ = _iteration(False, tg.StepOptions())
    assert "vgg_loss" in out0 and "vgg_loss" not in out_off
    assert abs(out0["errG"].item() - out_off["errG"].item()) <= 1e-5 * abs(out_off["errG"].item()) + 1e-6
    bar, worst = (1e-5 if mode == "fp32" else 2.0 ** -8), 0.0
    for k, g_off in grads_off[0].items():
        g0 = grads_zero[0][k]
        assert (g0 is None) == (g_off is None), k
        if g_off is not None:
            e = ((g0 - g_off).norm() / g_off.norm().clamp_min(1e-30)).item()
            worst = max(worst, e)
            assert e <= bar, (k, e)
    moved = max(((grads_on[0][k] - g).norm() / g.norm().clamp_min(1e-30)).item() for k, g in grads_off[0].items() if g is not None)
    print(f"[vgg iteration {mode}] generator gradients, smooth 0 vs E.VGG off: worst tensor {worst:.2e} (bar {bar:.1e}); smooth 1 moves them by {moved:.2e}")
    assert moved > worst                                      # and at weight 1 the term does reach the generator


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_graph_replay_gives_the_eager_iterations_vgg_loss_bytes(mode, weights_file):
    """under ops.fixed_order(), the third iteration of a `GraphedIteration` (two eager warm-ups, then capture + replay: the term runs inside
    the captured graph, on weights packed before it) against an eager iteration.  Learning rate 0 on both sides: the replayed iteration is
    then the SAME iteration as the eager one (the weight gradients' f32 atomics are not order-fixed, so after a real optimizer step two runs
    no longer hold the same weights), and vgg_loss, a forward quantity of fixed-order kernels, must be the same bytes."""
    import xmc_gan.train_gan as tg
    ops.set_precision(mode)
    contrast = VGGContrast(VGG19Features(weights_file, DEV).warm())
    with ops.fixed_order():
        eager, _, _, _ = _iteration(True, tg.StepOptions(vgg=contrast), lr=0.0)
        replay, _, _, replayed = _iteration(True, tg.StepOptions(vgg=contrast), lr=0.0, steps=3, graph=True)
    assert replayed
    print(f"\n[vgg graph replay {mode}] vgg_loss eager {eager['vgg_loss'].item():.9g}, replayed {replay['vgg_loss'].item():.9g}")
    assert torch.equal(eager["vgg_loss"], replay["vgg_loss"]) and torch.isfinite(replay["vgg_loss"])


def test_without_the_switch_the_launch_list_is_unchanged(monkeypatch, weights_file):
    """E.VGG off: the same library calls and the same convolution launches (family, shape tag, kernel instantiation), in the same order, with
    and without a VGG-19 in the step options, and none of csrc/vgg.hip's entry points among them; with the switch on they are there"""
    import xmc_gan.train_gan as tg
    ops.set_precision("bf16")
    contrast = VGGContrast(VGG19Features(weights_file, DEV).warm())
    calls = _Calls(monkeypatch)
    lists = []
    for opts in (tg.StepOptions(), tg.StepOptions(vgg=contrast)):
        del calls.names[:]
        prof.enable()
        try:
            out, _, _, _ = _iteration(False, opts)
            lists.append((list(calls.names), [(r.family, r.tag, r.kernel) for r in prof.launches()]))
        finally:
            prof.disable()
        assert "vgg_loss" not in out and calls.vgg() == []
    assert lists[0] == lists[1] and len(lists[0][0]) > 50 and len(lists[0][1]) > 20
    del calls.names[:]
    out, _, _, _ = _iteration(True, tg.StepOptions(vgg=contrast))
    # two forwards (real, generated) and one backward: prep 2 + 1, pools 2 * 5 + 5
    assert "vgg_loss" in out and sorted(set(calls.vgg())) == ["xmc_relu_maxpool2_bwd", "xmc_relu_maxpool2_fwd", "xmc_vgg_prep_bwd", "xmc_vgg_prep_fwd"]
    assert [calls.vgg().count(n) for n in ("xmc_vgg_prep_fwd", "xmc_vgg_prep_bwd", "xmc_relu_maxpool2_fwd", "xmc_relu_maxpool2_bwd")] == [2, 1, 10, 5]


def test_the_switch_without_a_network_is_refused(weights_file):
    import xmc_gan.train_gan as tg
    ops.set_precision("bf16")
    with pytest.raises(ImportError, match="--vgg_weights"):
        _iteration(True, tg.StepOptions())
