"""The entry of a generator block with a learned shortcut as one pass over the block input per direction (xmc_gentry_fwd /
xmc_gentry_bwd, csrc/conv_thin.hip; ops._engine._gentry_fwd_raw / _gentry_bwd_raw, ops.GBlockEntryFn) against

  * the launches it replaces (what XMC_DEBUG_DISPATCH=no_gentry_fused runs): `_affine_fwd_raw`, the 1x1 forward, `_conv_dgrad_raw` of
    the 1x1 and `_affine_bwd_raw(..., dx_acc=dskip, want_sumpool=pool)`.  h, sc, dx and the pooled dx bit for bit; the four per-sample
    sums, whose f32 additions run in another order, within `R.red_bound` of the f64 reference at the NEW kernel's reduction depth
    (`gentry_bwd_geom` below restates its loops);
  * f64 on the CPU: sc = x w^T + b and dskip = dsc w of the rounded operands, dskip rounded to the storage format, the rest through
    `R.affine_ref(..., dx_in=dskip)`.  Where the kernel's f32 dskip may round to the other neighbour than the f64 one (the MFMAs add K
    products in f32: |error| <= g(K) A), dx may move by that step and by one more rounding of its own: `flip` below, zero for nearly
    every element.

Shapes (N, H, W) at the three channel pairs the kernels are built for: one 16-pixel group; 60 pixels per image (groups straddle rows,
the last group of an image is partial, the pooled form has 15 quads: a partial group of quads); 96 pixels; 512 pixels with a grid_cap
that makes every workgroup walk several groups of both images.  BIG: the smallest shapes at which today's 1x1 launches are the streaming
kernels (pw1x1_kernel from 16384 pixels, pw1x1w_kernel from 32768) that the training step replaces: bit equality only."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointwise_ref as R

if torch.cuda.is_available():
    from xmc_gan_amd import ops
    from xmc_gan_amd import lib as L
    from xmc_gan_amd.ops import _engine as E
    from xmc_gan_amd.ops import _nodes_block as NB
    from test_ops_gpu import tol

DEV = "cuda"
PAIRS = [(64, 32), (128, 64), (256, 128)]
SHAPES = [(1, 2, 8, 0), (3, 6, 10, 0), (2, 8, 12, 0), (2, 16, 32, 3)]          # N, H, W, grid_cap
BIG = {(64, 32): (4, 64, 64), (128, 64): (4, 64, 64), (256, 128): (8, 64, 64)}
MODES = ["bf16", "f16"]
RESIDENT_MIN = 256                       # at least one workgroup per compute unit is resident


@pytest.fixture(autouse=True)
def _restore_precision():
    yield
    ops.set_precision("bf16")
    ops.precise_trunk(None)


def dev(t, mode=None):
    return t.to(R.DTYPE[mode] if mode else torch.float32).to(DEV).contiguous()


def bits(t):
    return t.contiguous().view(torch.int16)


def gentry_bwd_geom(N, H, W, Cin, pool, cap=0):
    """xmc_gentry_bwd restated: groups of 16 pixels (pool: four quads) per image, a contiguous run of groups per workgroup, its waves
    taking them in turn; a lane adds C8 / 4 pixels per group, the wave's pixel lanes meet in log2(64 / C8) exchanges, and every wave
    adds its sums of an image with one atomic.  depth: the longest such chain of additions over the images."""
    C8 = Cin // 8
    nw = 8 if Cin == 256 else 4
    gpi = R.cdiv((H // 2) * (W // 2), 4) if pool else R.cdiv(H * W, 16)
    nvg = N * gpi
    assert cap or nvg <= RESIDENT_MIN, "the grid of this shape depends on the device"
    gx = min(cap or RESIDENT_MIN, nvg)
    per = R.cdiv(nvg, gx)
    grid = R.cdiv(nvg, per)
    depth = groups_per_wave = 0
    for n in range(N):
        flushes = most = 0
        for b in range(grid):
            for w in range(nw):
                mine = [g for g in range(b * per + w, min((b + 1) * per, nvg), nw) if g // gpi == n]
                flushes += bool(mine)
                most = max(most, len(mine))
        depth = max(depth, most * (C8 // 4) + int(math.log2(64 // C8)) + flushes)
        groups_per_wave = max(groups_per_wave, most)
    return dict(gpi=gpi, nvg=nvg, grid=grid, per=per, groups_per_wave=groups_per_wave, depth=depth)


def make_case(N, H, W, cin, cout, mode, mutate=None):
    """f64 operands already representable in the storage format: x (kink-free), ps, dy, dsc, and the f32 parameters w, b"""
    g = R.gen_for("gentry", N, H, W, cin, cout, mode, mutate)
    x, ps, dy, _ = R.affine_inputs(g, (N, H, W, cin), mode)
    if mutate == "params":               # the vectors of image 0 and image 1 far apart: a parameter set of the wrong image shows
        ps = [t.clone() for t in ps]
        ps[0][0] *= 4.0
        ps[2][0] *= -3.0
        ps[1][0] += 2.0
        x = R.fix_kinks(x, lambda t: R.affine_pre(t, ps), mode)
    dsc = R.randn(g, (N, H, W, cout), mode)
    if mutate == "dsc":                  # dsc on a single pixel of the last image: a wrong group-to-image mapping moves dx by whole terms
        keep = torch.zeros(N, H, W, 1, dtype=torch.float64)
        keep[N - 1, H - 1, W // 2] = 1.0
        dsc = dsc * keep
    w = R.rand_f32(g, (cout, cin), cin ** -0.5)
    b = R.rand_f32(g, (cout,), 0.1)
    return x, ps, dy, dsc, w, b


def on_device(case, mode):
    x, ps, dy, dsc, w, b = case
    cout, cin = w.shape
    wp = torch.nn.Parameter(w.float().reshape(cout, cin, 1, 1).to(DEV))
    return dev(x, mode), [dev(t) for t in ps], dev(dy, mode), dev(dsc, mode), wp, dev(b), ops.ConvGeom(cin, cout, 1, 1, 0)


def today(xd, psd, dyd, dscd, wp, bd, geom, pool):
    """the four launches the fused kernels replace"""
    H, W = xd.shape[1], xd.shape[2]
    h = E._affine_fwd_raw(xd, psd, 0.2)
    sc = E._conv_fwd_raw(xd, wp, bd, geom, L.ACT_NONE, xd.dtype)
    dskip = E._conv_dgrad_raw(dscd, wp, geom, (H, W), xd.dtype)
    r = E._affine_bwd_raw(xd, dyd, psd, 0.2, dx_acc=dskip, want_sumpool=pool)
    return h, sc, r[0], r[1], (r[2] if pool else None)


def reference(case, mode, pool):
    x, ps, dy, dsc, w, b = case
    K = w.shape[0]
    wq = R.rt(w, mode)
    sc, A_sc = x @ wq.t() + b, x.abs() @ wq.abs().t() + b.abs()
    dskip, A_dskip = dsc @ wq, dsc.abs() @ wq.abs()
    d = R.gamma(K) * A_dskip
    flip = (R.rt(dskip + d, mode) - R.rt(dskip - d, mode)).abs()              # the step dskip's rounding may take the other way
    ref = R.affine_ref(x, ps, mode, dy, dx_in=R.rt(dskip, mode), pool=pool)
    return dict(sc=sc, A_sc=A_sc, flip=flip, **ref)


def check_elem(got, ref, A, mode, what, extra=0.0):
    err = (got.detach().double().cpu().reshape(ref.shape) - ref).abs()
    bound = R.elem_bound(ref, A, mode) + extra
    ratio = float((err / bound).max())
    print(f"{what}: worst |got - ref| / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: {int((err > bound).sum())} of {err.numel()} elements beyond the bound, worst ratio {ratio:.3f}"


def check_sums(red, ref, depth, what):
    for i, (val, S) in enumerate(ref["grads"]):
        err = (red[i].detach().double().cpu() - val).abs()
        bound = R.red_bound(S, depth, R.AFFINE_GRAD_OPS) + 1e-300
        ratio = float((err / bound).max())
        print(f"{what} {('dg0', 'db0', 'dg1', 'db1')[i]}: worst |got - ref| / bound = {ratio:.3f} at depth {depth}")
        assert ratio <= 1.0, f"{what} sum {i}: worst ratio {ratio:.3f}"


def run_case(N, H, W, cap, cin, cout, mode, mutate=None):
    ops.set_precision(mode)
    case = make_case(N, H, W, cin, cout, mode, mutate)
    xd, psd, dyd, dscd, wp, bd, geom = on_device(case, mode)
    what = f"gentry {cin}->{cout} N{N} {H}x{W} cap={cap} {mode} mutate={mutate}"
    ops.new_iteration(DEV)
    fwd = E._gentry_fwd_raw(xd, psd, wp, bd, geom, grid_cap=cap)
    assert fwd is not None, "the fused forward declined a shape it is built for"
    assert L.load().xmc_last_kernel().decode().startswith("gentry_fwd_kernel")
    for pool in ((False, True) if H % 2 == 0 and W % 2 == 0 else (False,)):
        t_h, t_sc, t_dx, t_red, t_dxp = today(xd, psd, dyd, dscd, wp, bd, geom, pool)
        bwd = E._gentry_bwd_raw(xd, dyd, dscd, psd, wp, geom, want_sumpool=pool, grid_cap=cap)
        assert bwd is not None, "the fused backward declined a shape it is built for"
        assert L.load().xmc_last_kernel().decode().startswith("gentry_bwd_kernel")
        dx, red, dxp = bwd
        # (1) today's sequence, bit for bit
        assert torch.equal(bits(fwd[0]), bits(t_h)), what + ": h differs from xmc_affine2_act_fwd"
        assert torch.equal(bits(fwd[1]), bits(t_sc)), what + ": sc differs from the 1x1 forward"
        assert torch.equal(bits(dx), bits(t_dx)), what + f": dx differs from the unfused sequence (pool={pool})"
        if pool:
            assert torch.equal(bits(dxp), bits(t_dxp)), what + ": the pooled dx differs from the unfused sequence"
        # (2) f64
        ref = reference(case, mode, pool)
        geo = gentry_bwd_geom(N, H, W, cin, pool, cap)
        check_elem(fwd[0], ref["y"], ref["A_y"], mode, what + " h")
        check_elem(fwd[1], ref["sc"], ref["A_sc"], mode, what + " sc", extra=R.gamma(cin) * ref["A_sc"])
        moved = (ref["flip"] > 0).double() * (ref["flip"] + 2.0 * R.U_FMT[mode] * (ref["dx"].abs() + ref["flip"]))
        check_elem(dx, ref["dx"], ref["A_dx"], mode, what + f" dx pool={pool}", extra=moved)
        check_sums(red, ref, geo["depth"], what + f" pool={pool}")
        check_sums(t_red, ref, R.affine_bwd_geom(N, H, W, cin, pool)["depth_param"], what + f" pool={pool} (unfused)")
        if pool:
            extra = ref["slack_pool"] + R.sumpool2_ref(moved, 1.0)[0]
            check_elem(dxp, ref["pool"], ref["A_pool"], mode, what + " pooled dx", extra=extra)
    return geo


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cin,cout", PAIRS)
@pytest.mark.parametrize("N,H,W,cap", SHAPES)
def test_fused_entry_against_unfused_and_f64(N, H, W, cap, cin, cout, mode):
    geo = run_case(N, H, W, cap, cin, cout, mode)
    if cap:
        assert geo["grid"] == cap and geo["groups_per_wave"] >= 2, "the capped grid must make a wave walk several groups"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cin,cout", PAIRS)
@pytest.mark.parametrize("mutate", ["dsc", "params"])
def test_fused_entry_mutations(mutate, cin, cout, mode):
    """dsc on one pixel of the last image / the parameters of image 0 far from image 1's, at 60 pixels per image (3 images: groups of
    one image end inside a workgroup's run), two workgroups"""
    run_case(3, 6, 10, 2, cin, cout, mode, mutate)


@pytest.mark.parametrize("cin,cout", PAIRS)
def test_fused_entry_bits_where_the_streaming_1x1_kernels_run(cin, cout):
    """the shapes from which today's 1x1 launches are pw1x1_kernel / pw1x1w_kernel, the kernels the training step's launches are:
    h, sc, dx and the pooled dx keep their bits"""
    ops.set_precision("bf16")
    N, H, W = BIG[(cin, cout)]
    g = torch.Generator().manual_seed(cin)
    rnd = lambda *sh, sc=1.0: (torch.randn(*sh, generator=g) * sc).to(DEV)
    xd, dyd, dscd = (rnd(N, H, W, c).to(torch.bfloat16) for c in (cin, cin, cout))
    psd = [rnd(N, cin, sc=0.5) + s for s in (1.0, 0.0, -1.0, 0.0)]
    wp, bd, geom = torch.nn.Parameter(rnd(cout, cin, 1, 1, sc=cin ** -0.5)), rnd(cout, sc=0.1), ops.ConvGeom(cin, cout, 1, 1, 0)
    ops.new_iteration(DEV)
    t_h, t_sc, t_dx, t_red, t_dxp = today(xd, psd, dyd, dscd, wp, bd, geom, True)
    h, sc = E._gentry_fwd_raw(xd, psd, wp, bd, geom)
    dx, red, dxp = E._gentry_bwd_raw(xd, dyd, dscd, psd, wp, geom, want_sumpool=True)
    for got, want, name in ((h, t_h, "h"), (sc, t_sc, "sc"), (dx, t_dx, "dx"), (dxp, t_dxp, "pooled dx")):
        assert torch.equal(bits(got), bits(want)), f"{cin}->{cout} N{N} {H}x{W}: {name} differs from the unfused sequence"
    torch.testing.assert_close(red, t_red, **tol("bf16", float(t_red.abs().max())))


@pytest.mark.parametrize("mode", MODES)
def test_fused_entry_with_a_gradient_absent(mode, monkeypatch):
    """GBlockEntryFn keeps set_materialize_grads(False): with dy absent the shortcut's gradient alone comes back, with dsc absent the
    plain affine backward runs; neither launches the fused backward"""
    ops.set_precision(mode)
    N, H, W, cin, cout = 2, 8, 12, 64, 32
    case = make_case(N, H, W, cin, cout, mode)
    xd, psd, dyd, dscd, wp, bd, geom = on_device(case, mode)
    bp = torch.nn.Parameter(bd)
    calls = []
    monkeypatch.setattr(NB, "_gentry_bwd_raw", lambda *a, **k: calls.append(1) or E._gentry_bwd_raw(*a, **k))
    for which in ("dsc only", "dy only", "both"):
        x = xd.clone().requires_grad_()
        ps = [t.clone().requires_grad_() for t in psd]
        wp.grad = bp.grad = None
        h, sc = ops.g_block_entry(x, ps, wp, bp, geom, True)
        ops.new_iteration(DEV)
        del calls[:]
        if which == "dsc only":
            sc.backward(dscd)
            assert not calls and ps[0].grad is None
            assert torch.equal(bits(x.grad), bits(E._conv_dgrad_raw(dscd, wp, geom, (H, W), xd.dtype)))
            assert wp.grad is not None and bp.grad is not None
        elif which == "dy only":
            h.backward(dyd)
            assert not calls and wp.grad is None and bp.grad is None
            t_dx, t_red, _ = E._affine_bwd_raw(xd, dyd, psd, 0.2, want_sumpool=True)
            assert torch.equal(bits(x.grad), bits(t_dx))
            check_sums([t.grad for t in ps], R.affine_ref(case[0], case[1], mode, case[2]), R.affine_bwd_geom(N, H, W, cin, True)["depth_param"], which)
        else:
            torch.autograd.backward([h, sc], [dyd, dscd])
            assert calls
            assert torch.equal(bits(x.grad), bits(today(xd, psd, dyd, dscd, wp, bd, geom, True)[2]))


def test_fused_entry_declines(monkeypatch):
    """odd H with the pool, f32 storage, the precise trunk's weight pair, other channel counts and the debug token: None, nothing
    launched, nothing written"""
    ops.set_precision("bf16")
    case = make_case(2, 5, 8, 64, 32, "bf16")
    xd, psd, dyd, dscd, wp, bd, geom = on_device(case, "bf16")
    lib = L.load()
    dx = torch.full_like(xd, 768.0)
    dxp = torch.full((2, 2, 4, 64), 768.0, dtype=xd.dtype, device=DEV)
    red = torch.zeros(4, 2, 64, device=DEV)
    wpk = E._packed_cached(wp, geom, 1, xd.dtype)
    p = ops._p
    rc = lib.xmc_gentry_bwd(p(xd), p(dyd), p(dscd), *[p(t) for t in psd], p(wpk), p(dx), p(dxp), *[p(red[i]) for i in range(4)],
                            2, 5, 8, 64, 32, wpk.shape[1], 0.2, ops._code(xd.dtype), 0, ops._st())
    torch.cuda.synchronize()
    assert rc == 1 and bool((dx == 768.0).all()) and bool((dxp == 768.0).all()) and float(red.abs().max()) == 0.0
    assert E._gentry_bwd_raw(xd, dyd, dscd, psd, wp, geom, want_sumpool=True) is None
    assert E._gentry_bwd_raw(xd, dyd, dscd, psd, wp, geom, want_sumpool=False) is not None           # without the pool odd sizes are taken
    assert E._gentry_fwd_raw(xd, psd, wp, bd, geom, pair=True) is None
    g32 = ops.ConvGeom(32, 32, 1, 1, 0)
    assert E._gentry_fwd_raw(xd[..., :32].contiguous(), [t[:, :32].contiguous() for t in psd], wp, bd, g32) is None
    ops.set_precision("fp32")
    assert E._gentry_fwd_raw(xd.float(), psd, wp, bd, geom) is None
    assert ops.g_block_entry(xd.float(), psd, wp, bd, geom) is None
    ops.set_precision("bf16")
    monkeypatch.setattr(E, "_DEBUG_DISPATCH", frozenset({"no_gentry_fused"}))
    assert E._gentry_fwd_raw(xd, psd, wp, bd, geom) is None and ops.g_block_entry(xd, psd, wp, bd, geom) is None


def sum_magnitudes(x, ps, dy, slope=R.SLOPE):
    """S of the four sums as `R.affine_ref` forms it, for an x that was not made kink-free (both kernels evaluate the pre-activations
    with the same instructions, so a value next to a kink falls on the same side in both)"""
    e = lambda t: t[:, None, None, :]
    u = x * e(ps[0]) + e(ps[1])
    su = torch.where(u > 0, 1.0, slope)
    a1, A_a1 = u * su, ((x * e(ps[0])).abs() + e(ps[1]).abs()) * su
    sv = torch.where(a1 * e(ps[2]) + e(ps[3]) > 0, 1.0, slope)
    dvv = dy * sv
    du = dvv * e(ps[2]) * su
    red = lambda t: t.sum((1, 2))
    return [red((du * x).abs()), red(du.abs()), red(dvv.abs() * A_a1), red(dvv.abs())]


def _block_grads(dt, seed):
    from xmc_gan.model.df_gan import G_Block
    N, H, W, cin, cout = 2, 8, 12, 64, 32
    torch.manual_seed(seed)
    blk = G_Block(cin, cout, 16, True).to(DEV)
    with torch.no_grad():
        blk.gamma.fill_(0.7)
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *sh, sc=1.0: (torch.randn(*sh, generator=g) * sc).to(DEV)
    x = rnd(N, H, W, cin).to(dt).requires_grad_()
    mod = [(rnd(N, c, sc=0.5) + (1.0 if i % 2 == 0 else 0.0)).requires_grad_() for i, c in enumerate([cin] * 4 + [cout] * 4)]
    r = rnd(N, 2 * H, 2 * W, cout)
    out = blk.forward_fused(x, mod, True, x_from_end=True)
    ops.new_iteration(DEV)
    (out.float() * r).sum().backward()
    return x, mod, {n: p_.grad for n, p_ in blk.named_parameters() if p_.grad is not None}, None


@pytest.mark.parametrize("no_wgrad", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_block_with_and_without_the_fused_entry(mode, no_wgrad, monkeypatch):
    """G_Block.forward_fused with a pending upsample, as the generator calls it, against the same block under no_gentry_fused: the input
    gradient and c_sc's weight and bias gradient (the same launch on the same operands) to the bit, the four sums within the sum of
    both kernels' bounds, every other parameter gradient -- same kernels on bit-identical operands, atomics in any order -- within the
    weight-gradient tolerance of test_ops_gpu"""
    import contextlib
    ops.set_precision(mode)
    ops.precise_trunk(False)          # (the IEEE-half mode's default keeps c_sc on its weight pair: the entry then declines, as tested above)
    dt = ops.act_dtype()
    seen = {}
    real_f = NB._gentry_bwd_raw
    monkeypatch.setattr(NB, "_gentry_bwd_raw", lambda x, dy, dsc, *a, **k: seen.update(fused=(x, dy)) or real_f(x, dy, dsc, *a, **k))
    with (ops.no_wgrad() if no_wgrad else contextlib.nullcontext()):
        xn, modn, gn, _ = _block_grads(dt, 5)
        assert "fused" in seen, "the block did not take the fused entry"
        monkeypatch.setattr(E, "_DEBUG_DISPATCH", frozenset({"no_gentry_fused"}))
        monkeypatch.setattr(NB, "_gentry_bwd_raw", lambda *a, **k: pytest.fail("fused backward under no_gentry_fused"))
        xo, modo, go, _ = _block_grads(dt, 5)
    assert torch.equal(bits(xn.grad), bits(xo.grad)), "the block input's gradient"
    assert set(gn) == set(go)
    assert "c_sc.weight" in gn or no_wgrad           # (inside no_wgrad() the two paths skip the same gradients, if any)
    for n in gn:
        if n.startswith("c_sc."):
            assert torch.equal(gn[n], go[n]), n
        else:
            torch.testing.assert_close(gn[n], go[n], **tol(mode, float(go[n].abs().max())))
    for i in range(4, 8):
        torch.testing.assert_close(modn[i].grad, modo[i].grad, **tol(mode, float(modo[i].grad.abs().max())))
    # the four sums: both within their own bound of the exact sums, whose term magnitudes S come from the f64 reference on what the
    # fused backward was handed
    x64, dy64 = seen["fused"][0].detach().double().cpu(), seen["fused"][1].detach().double().cpu()
    N, H, W, cin = x64.shape
    dn, do = gentry_bwd_geom(N, H, W, cin, True)["depth"], R.affine_bwd_geom(N, H, W, cin, True)["depth_param"]
    for i, S in enumerate(sum_magnitudes(x64, [t.detach().double().cpu() for t in modn[:4]], dy64)):
        bound = R.red_bound(S, dn, R.AFFINE_GRAD_OPS) + R.red_bound(S, do, R.AFFINE_GRAD_OPS) + 1e-300
        ratio = float(((modn[i].grad.double().cpu() - modo[i].grad.double().cpu()).abs() / bound).max())
        print(f"sum {i}: |fused - unfused| / bound = {ratio:.3f}")
        assert ratio <= 1.0
