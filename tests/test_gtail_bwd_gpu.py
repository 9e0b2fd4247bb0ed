"""The backward of the generator's tail (LeakyReLU -> conv_out -> tanh) as one pass over conv_out's input (xmc_gtail_bwd,
csrc/conv_thin.hip gtail_bwd_kernel; ops._engine._gtail_bwd_raw, ops.GBlockEndFn.backward) against

  * the three launches it replaces (xmc_tanh_bwd, the 32 -> 3 weight gradient, the masked and pooled data gradient; what
    XMC_DEBUG_DISPATCH=no_gtail_fused runs): dz and its 2x2 sum pool bit for bit, dW and db within the weight-gradient bound of
    test_ops_gpu.test_conv_fwd_dgrad_wgrad (`tol`: only the order of the f32 additions differs);
  * autograd through LeakyReLU, F.conv2d and tanh in f32 on the CPU, on the same rounded operands, within the same bounds.

Shapes: the kernel tiles 8x32 pixels and pools 2x2 -- one tile with an all-zero halo; a partial tile in x with tiles of several
images per workgroup; more tiles than workgroups (``grid_cap``), so that the accumulators live across tiles."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from xmc_gan_amd import ops
    from xmc_gan_amd import lib as L
    from xmc_gan_amd.ops import _engine as E
    from xmc_gan_amd.ops._config import _code, _p, _st
    from test_ops_gpu import from_nhwc, rt, to_nhwc, tol

DEV = "cuda"
# N, H, W, grid_cap (0: the launcher's own grid, one tile per workgroup at these sizes)
SHAPES = [(1, 8, 32, 0), (3, 24, 40, 0), (3, 24, 40, 4), (2, 64, 64, 0), (2, 64, 64, 16)]


def _inputs(N, H, W, cin, mode, seed, mutate=False):
    """CPU f32 operands already rounded to the storage format: z (the block sum), y = LeakyReLU(z) as stored, w, b, the tanh image
    and the gradient dy of that image"""
    g = torch.Generator().manual_seed(seed)
    z = rt(torch.randn(N, cin, H, W, generator=g), mode)
    y = rt(F.leaky_relu(z, 0.2), mode)
    w = rt(torch.randn(3, cin, 3, 3, generator=g) * (9 * cin) ** -0.5, mode)
    b = torch.randn(3, generator=g) * 0.1
    img = rt(torch.tanh(F.conv2d(y, w, b, 1, 1)), mode)
    dy = rt(torch.randn(N, 3, H, W, generator=g), mode)
    if mutate:
        # tanh' = 0 on a third of the pixels, dy only on the image border: a wrong halo or tap shift moves dW by whole terms
        sat = torch.rand(N, 1, H, W, generator=g) < 0.33
        img = torch.where(sat, torch.sign(img) + (img == 0).float(), img)
        border = torch.zeros(1, 1, H, W)
        border[..., 0, :] = border[..., -1, :] = border[..., :, 0] = border[..., :, -1] = 1.0
        dy = dy * border
    return z, y, w, b, img, dy


def _device(y, w, img, dy, dt):
    cin = y.shape[1]
    geom = ops.ConvGeom(cin, 3, 3, 1, 1)
    return (to_nhwc(dy, 8, dt), to_nhwc(img, 8, dt), to_nhwc(y, ops.chan_pad(cin, dt), dt), torch.nn.Parameter(w.to(DEV)), geom)


def _today(dyd, imgd, yd, wd, geom, want_w=True):
    """the three launches of GBlockEndFn.backward's unfused tail"""
    N, H, W, _ = yd.shape
    dpre = torch.empty_like(dyd)
    L.call("xmc_tanh_bwd", _p(dyd), _p(imgd), _p(dpre), dyd.numel(), _code(dyd.dtype), _st())
    gw = gb = None
    if want_w:
        gw, gb = E._conv_wgrad_raw(yd, dpre, geom, want_bias=True)
    dz, dsc = E._conv_dgrad_raw(dpre, wd, geom, (H, W), yd.dtype, mask=yd, want_sumpool=True)
    return dz, dsc, gw, gb


def _cpu(z, y, w, b, img, dy, through_tanh):
    """f32 autograd: z -> LeakyReLU (its value replaced by the stored y) -> conv2d -> tanh.  ``through_tanh`` False: the image is
    given (the mutation case sets it to +-1 by hand), so dpre = dy * (1 - img^2) is written out and autograd starts at the convolution."""
    zr, wr, br = z.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    a = F.leaky_relu(zr, 0.2)
    a = a + (y - a).detach()
    pre = F.conv2d(a, wr, br, 1, 1)
    if through_tanh:
        (torch.tanh(pre) * dy).sum().backward()
    else:
        pre.backward(dy * (1.0 - img * img))
    return zr.grad, 4.0 * F.avg_pool2d(zr.grad, 2), wr.grad, br.grad


def _check(fused, today, cpu, mode, cin):
    dz, dsc, gw, gb = fused
    tz, tsc, tw, tb = today
    assert torch.equal(dz.view(torch.int16), tz.view(torch.int16)), "dz differs from the unfused sequence"
    assert torch.equal(dsc.view(torch.int16), tsc.view(torch.int16)), "the pooled dz differs from the unfused sequence"
    cz, csc, cw, cb = cpu
    torch.testing.assert_close(from_nhwc(dz, cin), cz, **tol(mode, cz.abs().max().item()))
    torch.testing.assert_close(from_nhwc(dsc, cin), csc, **tol(mode, csc.abs().max().item()))
    if gw is None:
        return
    sw, sb = cw.abs().max().item(), cb.abs().max().item()
    print(f"dW: |fused - unfused| {(gw - tw).abs().max().item():.3e}, |fused - cpu| {(gw.cpu() - cw).abs().max().item():.3e}, scale {sw:.3e}; "
          f"db: {(gb[:3] - tb[:3]).abs().max().item():.3e}, {(gb[:3].cpu() - cb).abs().max().item():.3e}, scale {sb:.3e}")
    torch.testing.assert_close(gw, tw, **tol(mode, sw))
    torch.testing.assert_close(gb[:3], tb[:3], **tol(mode, sb))
    torch.testing.assert_close(gw.cpu(), cw, **tol(mode, sw))
    torch.testing.assert_close(gb[:3].cpu(), cb, **tol(mode, sb))


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("mutate", [False, True])
@pytest.mark.parametrize("N,H,W,cap", SHAPES)
def test_fused_tail_backward(N, H, W, cap, mutate, mode):
    ops.set_precision(mode)
    try:
        dt = ops.act_dtype()
        z, y, w, b, img, dy = _inputs(N, H, W, 32, mode, 11 * N + H + W, mutate)
        dyd, imgd, yd, wd, geom = _device(y, w, img, dy, dt)
        ops.new_iteration(DEV)
        fused = E._gtail_bwd_raw(dyd, imgd, yd, wd, geom, want_w=True, want_bias=True, grid_cap=cap)
        assert fused is not None, "the fused kernel declined a shape it is built for"
        today = _today(dyd, imgd, yd, wd, geom)
        _check(fused, today, _cpu(z, y, w, b, img, dy, through_tanh=not mutate), mode, 32)
    finally:
        ops.set_precision("bf16")


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_fused_tail_backward_without_weight_gradient(mode):
    """the `no_wgrad()` variant: tanh' is still fused, dz and its pool are still today's bits, no weight gradient comes back"""
    ops.set_precision(mode)
    try:
        dt = ops.act_dtype()
        z, y, w, b, img, dy = _inputs(3, 24, 40, 32, mode, 5)
        dyd, imgd, yd, wd, geom = _device(y, w, img, dy, dt)
        ops.new_iteration(DEV)
        fused = E._gtail_bwd_raw(dyd, imgd, yd, wd, geom, want_w=False, want_bias=True, grid_cap=4)
        assert fused is not None and fused[2] is None and fused[3] is None
        assert L.load().xmc_last_kernel().decode() == "gtail_bwd_kernel<0>"
        _check(fused, _today(dyd, imgd, yd, wd, geom, want_w=False), _cpu(z, y, w, b, img, dy, True), mode, 32)
    finally:
        ops.set_precision("bf16")


def test_fused_tail_backward_declines():
    """8 input channels (the NCH = 8 configurations), the f32 mode and the debug token are not the kernel's: None, nothing launched"""
    z, y, w, b, img, dy = _inputs(2, 16, 32, 8, "bf16", 3)
    ops.set_precision("bf16")
    dyd, imgd, yd, wd, geom = _device(y, w, img, dy, ops.act_dtype())
    assert E._gtail_bwd_raw(dyd, imgd, yd, wd, geom, want_w=True, want_bias=True) is None
    ops.set_precision("fp32")
    try:
        z, y, w, b, img, dy = _inputs(1, 8, 32, 32, "fp32", 3)
        dyd, imgd, yd, wd, geom = _device(y, w, img, dy, ops.act_dtype())
        assert E._gtail_bwd_raw(dyd, imgd, yd, wd, geom, want_w=True, want_bias=True) is None
    finally:
        ops.set_precision("bf16")


def _block_end_grads(C, N, H, W, dt, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *sh, sc=1.0: (torch.randn(*sh, generator=g) * sc).to(DEV)
    h1 = rnd(N, H, W, C).to(dt).requires_grad_()
    sc = rnd(N, H // 2, W // 2, C).to(dt).requires_grad_()
    ms = [(rnd(N, C, sc=0.5) + (1.0 if i % 2 == 0 else 0.0)).requires_grad_() for i in range(4)]
    w2, b2 = torch.nn.Parameter(rnd(C, C, 3, 3, sc=(9 * C) ** -0.5)), torch.nn.Parameter(rnd(C, sc=0.1))
    wo, bo = torch.nn.Parameter(rnd(3, C, 3, 3, sc=(9 * C) ** -0.5)), torch.nn.Parameter(rnd(3, sc=0.1))
    gam = torch.nn.Parameter(torch.full((1,), 0.7, device=DEV))
    r_img = rnd(N, H, W, 8).to(dt)
    y = ops.g_block_end(h1, ms, w2, b2, ops.ConvGeom(C, C, 3, 1, 1), sc, gam, tail=(wo, bo, ops.ConvGeom(C, 3, 3, 1, 1)))
    ops.new_iteration(DEV)
    (y.float() * r_img.float()).sum().backward()
    return h1.grad, sc.grad, wo.grad, bo.grad


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("C", [32, 8])
def test_block_end_node_with_and_without_the_fused_tail(C, mode, monkeypatch):
    """ops.g_block_end with the tail, as the generator calls it, against the same node under XMC_DEBUG_DISPATCH=no_gtail_fused: the
    gradients that depend on dz only through deterministic kernels (dh1, the shortcut's pooled gradient) keep their bits, conv_out's
    weight and bias gradient stay within the weight-gradient bound.  C = 8: the kernel declines, both runs take today's launches."""
    ops.set_precision(mode)
    try:
        dt = ops.act_dtype()
        new = _block_end_grads(C, 3, 32, 32, dt, 21)
        monkeypatch.setattr(E, "_DEBUG_DISPATCH", frozenset({"no_gtail_fused"}))
        old = _block_end_grads(C, 3, 32, 32, dt, 21)
        same = lambda a, b: torch.equal(a.view(torch.int16), b.view(torch.int16))
        assert same(new[1], old[1]), "the shortcut's gradient (the pooled output of the tail's data gradient)"
        assert same(new[0], old[0]), "dh1"
        torch.testing.assert_close(new[2], old[2], **tol(mode, old[2].abs().max().item()))
        torch.testing.assert_close(new[3], old[3], **tol(mode, old[3].abs().max().item()))
    finally:
        ops.set_precision("bf16")
