"""DiffAugment without a GPU: the f64 restatement the GPU tests compare the kernels with (tests/diffaug_ref.py) against torch autograd,
the host-side sampler (xmc_gan_amd/augment.py), and the entry point's flag."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diffaug_ref as R


def _rows():
    """N = 4 on a 6 x 5 map, cut = 3: a general row, a full shift-out (tx = -W), a cutout square hanging over two edges, the identity"""
    #                     b     s    c    tx  ty  cy  cx
    return torch.tensor([[0.3, 0.4, 1.3,  1, -2,  2,  1, 0],
                         [-0.2, 1.7, 0.6, -5,  0,  0,  0, 0],
                         [0.1, 0.0, 0.5,  0,  1,  4,  3, 0],
                         [0.0, 1.0, 1.0,  0,  0, -9, -9, 0]], dtype=torch.float64)


def test_restatement_transpose_is_autograd_of_its_forward():
    g = torch.Generator().manual_seed(1)
    N, C, H, W, cut = 4, 3, 6, 5, 3
    P = _rows()
    x = torch.randn(N, C, H, W, dtype=torch.float64, generator=g).requires_grad_()
    dy = torch.randn(N, C, H, W, dtype=torch.float64, generator=g)
    y = R.forward(x, P, cut)
    (auto,) = torch.autograd.grad(y, x, dy)
    err = (R.transpose(dy, P, cut) - auto).abs().max().item()
    print(f"\n[restatement] |A^T dy - autograd| = {err:.2e}")
    assert err <= 1e-12
    # the linear part is the forward without the b-term, and the forward is affine in x
    x2 = torch.randn(N, C, H, W, dtype=torch.float64, generator=g)
    assert (R.forward(x + x2, P, cut) - R.forward(x, P, cut) - R.linear(x2, P, cut)).abs().max().item() <= 1e-12
    # what the rows were chosen for
    assert R.forward(x, P, cut)[1].abs().max().item() == 0.0                   # shifted out of the frame entirely
    assert R.transpose(dy, P, cut)[1].abs().max().item() == 0.0                # ... so no dy reaches any of its sources (G = 0)
    assert R.transpose(dy, P, cut)[0][:, :, 0].abs().min().item() > 0.0        # tx = 1: column 0 feeds no output pixel but still the image mean
    assert torch.equal(R.forward(x, P, cut)[3], x[3].detach())                 # identity row
    assert R.forward(x, P, cut)[2][:, 4:6, 3:5].abs().max().item() == 0.0      # the square over the bottom-right corner
    # adjoint identity in f64
    lhs, rhs = (R.linear(x2, P, cut) * dy).sum().item(), (x2 * R.transpose(dy, P, cut)).sum().item()
    assert abs(lhs - rhs) <= 1e-12 * x2.abs().sum().item() * dy.abs().max().item()


def test_sampler_ranges_policy_and_seeding():
    from xmc_gan_amd.augment import DiffAugment, parse_policy
    H, W, n = 64, 48, 10000
    a = DiffAugment("color,translation,cutout", 4, H, W, "cpu", seed=7)
    rows = a.sample(n)
    assert rows.shape == (n, 8) and rows.dtype == torch.float32
    b, s, c, tx, ty, cy, cx, z = rows.unbind(1)
    assert (b >= -0.5).all() and (b < 0.5).all() and b.std() > 0.2
    assert (s >= 0).all() and (s < 2).all() and s.std() > 0.4
    assert (c >= 0.5).all() and (c < 1.5).all() and c.std() > 0.2
    rw, rh, cut = int(W * 0.125 + 0.5), int(H * 0.125 + 0.5), a.cut
    assert cut == int(min(H, W) * 0.5 + 0.5)
    for col in (tx, ty, cy, cx):
        assert torch.equal(col, col.round())                                   # exact integers stored as floats
    assert tx.min() == -rw and tx.max() == rw and ty.min() == -rh and ty.max() == rh
    assert cy.min() == -(cut // 2) and cy.max() == H + (1 - cut % 2) - 1 - cut // 2
    assert cx.min() == -(cut // 2) and cx.max() == W + (1 - cut % 2) - 1 - cut // 2
    assert (z == 0).all()
    # the device tensor: 3 * batch rows, identity until the first refresh, then a draw
    assert a.params.shape == (12, 8) and torch.equal(a.params, DiffAugment.identity_rows(12))
    a.refresh()
    assert not torch.equal(a.params, DiffAugment.identity_rows(12))
    assert a.rows_real().data_ptr() == a.params.data_ptr() and a.rows_d().shape == (8, 8)
    assert a.rows_fake().data_ptr() == a.params[4:].data_ptr() and a.rows_g().data_ptr() == a.params[8:].data_ptr()

    # components outside the policy keep their identity values
    ident = DiffAugment.identity_rows(n)
    t = DiffAugment("translation", 4, H, W, "cpu", seed=7)
    r = t.sample(n)
    assert torch.equal(r[:, :3], ident[:, :3]) and torch.equal(r[:, 5:], ident[:, 5:]) and t.cut == 0 and not t.color
    assert r[:, 3].abs().max() == rw
    k = DiffAugment("cutout,color", 4, H, W, "cpu", seed=7)
    r = k.sample(n)
    assert torch.equal(r[:, 3:5], ident[:, 3:5]) and k.cut == cut and k.color and k.policy == ("color", "cutout")

    # same seed -> same rows; another rank -> other rows; a resume seeds from the epoch as well
    mk = lambda **kw: DiffAugment("color,translation,cutout", 4, H, W, "cpu", **kw)
    assert torch.equal(mk(seed=3).sample(), mk(seed=3).sample())
    assert torch.equal(mk(seed=3, rank=0).sample(), mk(seed=3).sample())
    assert not torch.equal(mk(seed=3, rank=0).sample(), mk(seed=3, rank=1).sample())
    assert not torch.equal(mk(seed=3).sample(), mk(seed=4).sample())
    e = mk(seed=3)
    e.seed(3, 0, 52)
    assert not torch.equal(e.sample(), mk(seed=3).sample())

    with pytest.raises(ValueError):
        DiffAugment("color,flip", 4, H, W, "cpu", seed=1)
    with pytest.raises(ValueError):
        parse_policy("colour")
    assert parse_policy("") == () and parse_policy(None) == ()


def test_entry_point_flag():
    import xmc_gan.train_gan as tg
    assert tg.parse_args([]).diffaug == ""
    assert tg.parse_args(["--diffaug", "color"]).diffaug == "color"
    assert tg.StepOptions().diffaug is None
    with pytest.raises(SystemExit):
        tg.main(["--diffaug", "colour"])
