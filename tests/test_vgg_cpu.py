"""TRAIN.ENCODER_LOSS.VGG without a GPU: the loader and each of its refusals, the start-up refusal of the trainer, the C ABI's four new
entry points (named everywhere they must be, validating before any launch), and the pool's backward rule against torch.autograd."""
import ctypes
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import vgg_ref as R  # noqa: E402
import xmc_gan_amd.lib as L  # noqa: E402
from xmc_gan_amd import ops, vgg  # noqa: E402

ENTRY_POINTS = ("xmc_vgg_prep_fwd", "xmc_vgg_prep_bwd", "xmc_relu_maxpool2_fwd", "xmc_relu_maxpool2_bwd")


# ------------------------------------------------------------------------------------------ the layer plan and the loader
def test_layer_plan_is_torchvisions_vgg19():
    layers = vgg.vgg19_layers()
    assert tuple(i for i, _, _, _ in layers) == R.CONV_KEYS
    assert [c for _, _, c, _ in layers] == [v for v in R.PLAN if v != "M"] and layers[0][1] == 3
    assert [i for i, _, _, pooled in layers if pooled] == [2, 7, 16, 25, 34] and vgg.POOLS == 5 and vgg.DIMS == 512


def test_loader_round_trip(tmp_path):
    path = str(tmp_path / "vgg19.pth")
    weights = R.write_weights_file(path, seed=3)
    net = vgg.VGG19Features(path, device="cpu")
    assert len(net.layers) == 16
    for (geom, w, b, _), (w0, b0) in zip(net.layers, weights):
        assert isinstance(w, torch.nn.Parameter) and not w.requires_grad and not b.requires_grad
        assert (geom.cin, geom.cout, geom.k, geom.s, geom.p) == (w0.shape[1], w0.shape[0], 3, 1, 1)
        assert torch.equal(w, w0.float()) and torch.equal(b, b0.float())
    assert len(net.parameters()) == 32 and all(not p.requires_grad for p in net.parameters())


def test_loader_refusals(tmp_path):
    with pytest.raises(ImportError, match="does not exist"):
        vgg.VGG19Features(str(tmp_path / "nothing.pth"), device="cpu")
    path = str(tmp_path / "w.pth")
    R.write_weights_file(path, drop=("features.21.bias",))
    with pytest.raises(ImportError, match=r"lack 'features\.21\.bias'"):
        vgg.VGG19Features(path, device="cpu")
    R.write_weights_file(path, replace={"features.5.weight": torch.zeros(128, 64, 5, 5)})
    with pytest.raises(ValueError, match=r"features\.5\.weight.*\(128, 64, 5, 5\).*\(128, 64, 3, 3\)"):
        vgg.VGG19Features(path, device="cpu")
    R.write_weights_file(path, replace={"features.1.running_mean": torch.zeros(64)})
    with pytest.raises(NotImplementedError, match="vgg19_bn"):
        vgg.VGG19Features(path, device="cpu")
    torch.save([1, 2, 3], path)
    with pytest.raises(ImportError, match="state dict"):
        vgg.VGG19Features(path, device="cpu")


def test_sizes_that_five_pools_do_not_divide_are_refused(tmp_path):
    path = str(tmp_path / "w.pth")
    R.write_weights_file(path)
    net = vgg.VGG19Features(path, device="cpu")
    dt = ops.act_dtype()
    for hw in ((48, 64), (64, 80), (16, 16)):
        with pytest.raises(ValueError, match="multiples of 32"):
            net(torch.zeros(1, *hw, 8, dtype=dt))
    with pytest.raises(ValueError, match=r"\[N,H,W,8\]"):
        net(torch.zeros(1, 3, 64, 64, dtype=dt))
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # a size that fits gets as far as the first kernel
        net(torch.zeros(1, 64, 96, 8, dtype=dt))
    for fn in (ops.vgg_prep, ops.relu_maxpool2):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(torch.zeros(1, 4, 4, 8, dtype=dt))


# ------------------------------------------------------------------------------------------ the trainer's start-up refusal
def test_vgg_switch_without_weights_is_refused_at_start_up(tmp_path, monkeypatch):
    import xmc_gan.train_gan as tg
    from xmc_gan.config import gan
    yml = tmp_path / "vgg_on.yml"
    text = open(os.path.join(ROOT, "xmc_gan", "cfg", "df_gan_damsm.yml")).read()
    assert "VGG: false" in text
    yml.write_text(text.replace("VGG: false", "VGG: true"))
    monkeypatch.delenv("XMC_VGG19", raising=False)
    try:
        gan.reset_cfg()
        with pytest.raises(ImportError, match="--vgg_weights"):
            tg._checked_args(["--cfg", str(yml), "--synthetic", "2"])
        gan.reset_cfg()
        with pytest.raises(ImportError, match="--vgg_weights.*does not exist"):
            tg._checked_args(["--cfg", str(yml), "--synthetic", "2", "--vgg_weights", str(tmp_path / "nothing.pth")])
        gan.reset_cfg()
        path = str(tmp_path / "w.pth")
        R.write_weights_file(path)
        args, _, _ = tg._checked_args(["--cfg", str(yml), "--synthetic", "2", "--vgg_weights", path, "--vgg_smooth", "0.5"])
        assert args.vgg_weights == path and args.vgg_smooth == 0.5
        gan.reset_cfg()
        with pytest.raises(SystemExit, match="multiple of 32"):
            tg._checked_args(["--cfg", str(yml), "--synthetic", "2", "--vgg_weights", path, "--imsize", "80"])
        gan.reset_cfg()                      # without the switch nothing is looked for
        args, _, _ = tg._checked_args(["--cfg", os.path.join(ROOT, "xmc_gan", "cfg", "df_gan_damsm.yml"), "--synthetic", "2"])
        assert args.vgg_weights == "" and args.vgg_smooth == 1.0
    finally:
        gan.reset_cfg()
        ops.set_precision("bf16")
    opts = tg.StepOptions()
    assert opts.vgg is None and opts.vgg_smooth == 1.0


# ------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_are_named_in_every_layer():
    hdr = open(os.path.join(ROOT, "include", "xmc_gan_hip.h")).read()
    src = open(os.path.join(ROOT, "xmc-gan_amd", "csrc", "vgg.hip")).read()
    for n in ENTRY_POINTS:
        assert re.search(rf"^int {n}\(", hdr, re.M) and f'extern "C" int {n}(' in src and n in L.EXPORTS, n
    assert "vgg.hip" in re.search(r"^SRCS = (.*)$", open(os.path.join(ROOT, "xmc-gan_amd", "csrc", "Makefile")).read(), re.M).group(1)
    assert "atomic" not in src.split("#include")[1]                      # one writer per element, a fixed order
    for name in ("vgg_prep", "relu_maxpool2"):
        assert callable(getattr(ops, name)) and getattr(ops, name).__module__.endswith("ops._functional")
    for name in ("VggPrepFn", "VggPrepBwdFn", "ReluMaxPool2Fn", "ReluMaxPool2BwdFn"):
        assert getattr(ops, name).__module__.endswith("ops._nodes_leaf")
    for variant in ("bf16", "f16"):
        lib = L.load(variant)
        assert lib.xmc_abi_version() == 13 and all(hasattr(lib, n) for n in ENTRY_POINTS)


def test_entry_points_validate_before_any_launch():
    """NULL -> XMC_EINVAL, a shape that is not built -> XMC_ESHAPE, a misaligned pointer -> XMC_EALIGN: all three return before a launch, so
    they are checked here with made-up addresses that nothing dereferences"""
    A, B, D, M = (ctypes.c_void_p(a) for a in (1 << 20, 2 << 20, 3 << 20, (1 << 20) + 8))
    EINVAL, EALIGN, ESHAPE = -1, -2, -3
    cases = {       # name: (arguments that pass every check, [(index, value)] invalid / a shape that is not built / misaligned)
        "xmc_vgg_prep_fwd": ([A, B, 2, 4, 4, L.H16, None], [(0, None), (1, None), (5, 7)], [(2, 0), (3, 0), (4, 0)], [(0, M), (1, M)]),
        "xmc_vgg_prep_bwd": ([A, B, 2, 4, 4, L.F32, None], [(0, None), (1, None), (5, -1)], [(2, 0), (3, 0), (4, 0)], [(0, M), (1, M)]),
        "xmc_relu_maxpool2_fwd": ([A, B, 2, 4, 6, 24, L.H16, None], [(0, None), (1, None), (1, A), (6, 2)],
                                  [(2, 0), (3, 5), (4, 3), (3, 0), (5, 12), (5, 0), (5, 4)], [(0, M), (1, M)]),
        "xmc_relu_maxpool2_bwd": ([A, B, D, 2, 4, 6, 24, L.F32, None], [(0, None), (1, None), (2, None), (2, A), (2, B), (7, 2)],
                                  [(3, 0), (4, 5), (5, 3), (5, 0), (6, 12), (6, 0)], [(0, M), (1, M), (2, M)]),
    }
    assert set(cases) == set(ENTRY_POINTS)
    for variant in ("bf16", "f16"):
        lib = L.load(variant)
        for name, (good, invalid, shape, align) in cases.items():
            fn = getattr(lib, name)
            for rc, changes in ((EINVAL, invalid), (ESHAPE, shape), (EALIGN, align)):
                for i, v in changes:
                    args = list(good)
                    args[i] = v
                    assert fn(*args) == rc, (variant, name, i, v)
    big = 2 ** 31 - 1            # sizes whose product leaves 64 bits are refused like any other, not multiplied first
    assert lib.xmc_vgg_prep_fwd(A, B, big, big, big, L.F32, None) == ESHAPE
    assert lib.xmc_relu_maxpool2_bwd(A, B, D, big, big - 1, big - 1, big - 7, L.F32, None) == ESHAPE
    with pytest.raises(L.XmcHipError, match="XMC_ESHAPE"):
        L.check(L.load("bf16").xmc_relu_maxpool2_fwd(A, B, 1, 3, 4, 8, L.H16, None), "xmc_relu_maxpool2_fwd")


# ------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("shape", [(2, 8, 2, 2), (2, 24, 4, 6), (3, 8, 6, 4)])
def test_the_pool_backward_rule_is_torch_autograds_on_lattices_full_of_ties(shape):
    g = torch.Generator().manual_seed(sum(shape))
    z = torch.randint(-2, 3, shape, generator=g).double()
    z[0, 0, :2, :2] = -1.0                                   # an all-negative window
    z[0, 1, :2, :2] = torch.tensor([[-2.0, 0.0], [0.0, -1.0]])      # a maximum of exactly 0
    z[0, 2, :2, :2] = 2.0                                    # a four-way positive tie
    z.requires_grad_()
    p = F.relu(F.max_pool2d(z, 2))
    assert torch.equal(p, R.relu_maxpool2(z.detach()))
    dp = torch.randint(1, 5, p.shape, generator=g).double()
    (dz,) = torch.autograd.grad(p, z, dp)
    mine = R.relu_maxpool2_bwd(z.detach(), dp)
    assert torch.equal(mine, dz)
    assert mine[0, 0, :2, :2].abs().sum() == 0 and mine[0, 1, :2, :2].abs().sum() == 0
    assert mine[0, 2, 0, 0] == dp[0, 2, 0, 0] and mine[0, 2, :2, :2].sum() == dp[0, 2, 0, 0]


def test_the_restatement_is_differentiable_and_emulate_rounds_both_ways():
    weights = R.random_weights(1)
    x = (torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(2), dtype=torch.float64) * 2 - 1).requires_grad_()
    rows = R.forward(x, weights)
    assert rows.shape == (1, 512) and rows.dtype == torch.float64 and 0.05 < rows.abs().mean() < 20
    (gx,) = torch.autograd.grad(rows.sum(), x)
    assert gx.shape == x.shape and torch.isfinite(gx).all() and gx.abs().max() > 0
    assert R.forward(x.detach(), weights, stages=2).shape == (1, 128)
    x32 = x.detach().float().requires_grad_()
    rows16 = R.emulate(torch.bfloat16)(x32, weights)
    assert rows16.dtype == torch.float32
    err = ((rows16.double() - rows.detach()).abs().max() / rows.detach().pow(2).mean().sqrt()).item()
    assert 1e-4 < err < 0.2, err                             # eight significant bits through 16 layers: neither exact nor lost
    (g16,) = torch.autograd.grad(rows16.sum(), x32)
    assert torch.isfinite(g16).all()
    assert torch.equal(R.prep_bwd(torch.ones(1, 3, 2, 2, dtype=torch.float64)),
                       torch.autograd.grad(R.prep(x).sum(), x)[0][:, :, :2, :2])
