"""The kernels of csrc/pointwise.hip against the f64 references of tests/pointwise_ref.py, at the shapes where their launch geometry
changes (the case tables there; tests/test_pointwise_cpu.py holds every case to the regime it names).

Bounds are derived in pointwise_ref.py: one rounding to storage + 8 f32 operations per stored element, g(depth + ops) * sum|terms| per
f32 reduction with `depth` from the model of the launch, bit-equality for pure data movement.  None is a fraction of max|ref|.  The
small cases hold their reference on the host; the 8M- and 33M-element cases hold it in f64 on the device (ATen, not our kernels), where
it costs milliseconds.  Flat kernels write into a slice of a larger sentinel-filled buffer, so a store outside [0, n) is seen, and stays
inside memory the test owns."""
import ctypes as C
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointwise_ref as R

if torch.cuda.is_available():
    from xmc_gan_amd import lib as L
    from xmc_gan_amd import ops

DEV = "cuda"
SENT = 768.0                                   # exact in every format
GUARD = R.NT * R.UN * 8                        # elements on each side of a guarded output: one workgroup lap
PREFILL = 1.5


@pytest.fixture(autouse=True)
def _restore_precision():
    yield
    ops.set_precision("bf16")


def setup(mode):
    ops.set_precision(mode)
    dt = ops.act_dtype()
    return dt, ops._code(dt), ops._st()


def dev(t, mode=None):
    """a reference operand (f64, already representable) in the storage format on the device; mode None: f32"""
    return t.to(R.DTYPE[mode] if mode else torch.float32).to(DEV).contiguous()


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def guarded(n, dtype):
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf, n):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + n:] == SENT).all())


def f64(got, ref):
    return got.detach().double().to(ref.device).reshape(ref.shape)


def check_elem(got, ref, A, mode, what, extra_abs=0.0):
    err = (f64(got, ref) - ref).abs()
    bound = R.elem_bound(ref, A, mode, extra_abs)
    ratio = float((err / bound).max())
    print(f"{what}: worst |got - ref| / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: {int((err > bound).sum())} of {err.numel()} elements beyond the bound, worst ratio {ratio:.3f}"


def check_exact(got, ref, what):
    assert torch.equal(f64(got, ref), ref), f"{what}: not bit-exact"


def check_red(got, ref, S, depth, nops, what, slack=0.0):
    ref, S = torch.as_tensor(ref, dtype=torch.float64), torch.as_tensor(S, dtype=torch.float64)
    err = (f64(got, ref) - ref).abs()
    bound = R.red_bound(S, depth, nops, slack)
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: depth {depth}, worst |got - ref| / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: {int((err > bound).sum())} of {err.numel()} sums beyond the bound, worst ratio {ratio:.3f}"


# ------------------------------------------------------------------------------------------ flat maps and flat reductions
FLAT = [(n, m) for n in R.FLAT_SMALL for m in R.MODES] + [(R.FLAT_BIG, "bf16")]


@pytest.mark.parametrize("n,mode", FLAT)
def test_flat_maps(n, mode):
    dt, code, st = setup(mode)
    rdev = DEV if n == R.FLAT_BIG else None
    c = R.flat_case(n, mode, rdev)
    d = {k: dev(v, mode) for k, v in c.items()}
    al = torch.tensor([R.AL], dtype=torch.float32, device=DEV)
    sl = 0.2
    gen = R.gen_for("bits", n)
    bits = torch.randint(0, 256, (n // 8,), generator=gen, dtype=torch.int64).to(torch.uint8)
    bits_d = bits.to(DEV)
    on = ((bits.to(torch.int64)[:, None] >> torch.arange(8)) & 1).bool().reshape(n).to(c["dy"].device)
    y_lr, A_lr = R.lrelu_ref(c["x"])
    y_mk, A_mk = R.mask_ref(c["dy"], c["ref"])
    y_tb, A_tb = R.tanh_bwd_ref(c["dy"], c["y"])
    y_ax, A_ax = R.axpby_ref(c["x"], c["b"], R.AL)
    y_sg = torch.where(on, c["dy"], R.SLOPE * c["dy"])
    runs = [
        ("lrelu", lambda o: L.call("xmc_lrelu", p(d["x"]), p(o), n, sl, code, st), y_lr, A_lr, 0.0),
        ("tanh", lambda o: L.call("xmc_tanh", p(d["x"]), p(o), n, code, st), torch.tanh(c["x"]), torch.tanh(c["x"]).abs(), R.TANH_ABS),
        ("lrelu_mask", lambda o: L.call("xmc_lrelu_mask", p(d["dy"]), p(d["ref"]), p(o), n, sl, code, st), y_mk, A_mk, 0.0),
        ("tanh_bwd", lambda o: L.call("xmc_tanh_bwd", p(d["dy"]), p(d["y"]), p(o), n, code, st), y_tb, A_tb, 0.0),
        ("axpby", lambda o: L.call("xmc_axpby", p(d["x"]), p(d["b"]), p(al), p(o), n, code, st), y_ax, A_ax, 0.0),
        ("scale", lambda o: L.call("xmc_scale", p(d["x"]), p(al), p(o), n, code, st), R.AL * c["x"], (R.AL * c["x"]).abs(), 0.0),
        ("signmask_apply", lambda o: L.call("xmc_signmask_apply", p(d["dy"]), p(bits_d), p(o), n, sl, code, st), y_sg, y_sg.abs(), 0.0),
    ]
    for name, launch, ref, A, extra in runs:
        buf, out = guarded(n, dt)
        launch(out)
        check_elem(out, ref, A, mode, f"{name} n={n} {mode}", extra)
        assert guards_intact(buf, n), f"{name}: wrote outside its n = {n} elements"
    # reductions: accumulated into the caller's f32 scalar (pre-filled here: the += contract)
    g = R.stream_geom(n // 8)
    gr, A_gr, dot, S = R.scale_mask_dot_ref(c["dy"], c["ref"], R.AL)
    buf, out = guarded(n, dt)
    acc = torch.full((1,), PREFILL, dtype=torch.float32, device=DEV)
    L.call("xmc_scale_mask_dot", p(d["dy"]), p(d["ref"]), p(al), p(out), p(acc), n, code, st)
    check_elem(out, gr, A_gr, mode, f"scale_mask_dot g n={n} {mode}")
    assert guards_intact(buf, n)
    check_red(acc, [PREFILL + dot], [PREFILL + S], g["depth"] + 1, 1, f"scale_mask_dot dot n={n} {mode}")
    dot, S = R.dot_ref(c["x"], c["b"])
    acc = torch.full((1,), PREFILL, dtype=torch.float32, device=DEV)
    L.call("xmc_dot", p(d["x"]), p(d["b"]), p(acc), n, code, st)
    check_red(acc, [PREFILL + dot], [PREFILL + S], R.stride_geom(n // 8, 512)["depth"] + 1, 1, f"dot n={n} {mode}")


@pytest.mark.parametrize("n,variant", [(n, v) for n in R.FLAT_SMALL for v in ("bf16", "f16")] + [(R.FLAT_BIG, "bf16")])
def test_cast_all_four_dtype_pairs(n, variant):
    dt, h16, st = setup(variant)
    x32 = (torch.randn(n, generator=R.gen_for("cast", n)) * 3).to(DEV)
    xh = x32.to(dt)
    for src, dst, sc, dc in ((x32, torch.float32, L.F32, L.F32), (xh, dt, h16, h16), (xh, torch.float32, h16, L.F32), (x32, dt, L.F32, h16)):
        buf, out = guarded(n, dst)
        L.call("xmc_cast", p(src), p(out), n, sc, dc, st)
        what = f"cast {src.dtype} -> {dst} n={n}"
        if dst == torch.float32 or src.dtype == dst:
            check_exact(out, src.double(), what)                      # same or wider format: data movement
        else:
            check_elem(out, src.double(), torch.zeros_like(src, dtype=torch.float64), variant, what)
            check_exact(out, src.to(dst).double(), what + " (round to nearest even)")
        assert guards_intact(buf, n), what
    assert torch.equal(ops.cast(x32, dt), xh) and torch.equal(ops.cast(xh, torch.float32), xh.float())


@pytest.mark.parametrize("mode", R.MODES)
def test_flat_wrappers_through_autograd(mode):
    """ops.lrelu / ops.axpby (and their backward nodes) on the two-block size"""
    dt, code, st = setup(mode)
    n = 8 * 1025
    c = R.flat_case(n, mode)
    x = dev(c["x"], mode).view(1, 5, 41, 40).requires_grad_()
    b = dev(c["b"], mode).view(1, 5, 41, 40).requires_grad_()
    dy = dev(c["dy"], mode).view(1, 5, 41, 40)
    al = torch.nn.Parameter(torch.tensor([R.AL], device=DEV))
    y = ops.lrelu(x)
    check_elem(y, *R.lrelu_ref(c["x"]), mode, "ops.lrelu")
    (gx,) = torch.autograd.grad(y, x, dy)
    check_elem(gx, *R.mask_ref(c["dy"], c["x"]), mode, "ops.lrelu backward")
    z = ops.axpby(x, b, al)
    check_elem(z, *R.axpby_ref(c["x"], c["b"], R.AL), mode, "ops.axpby")
    ga, gb, gal = torch.autograd.grad(z, [x, b, al], dy)
    check_exact(ga, c["dy"], "ops.axpby d a")
    check_elem(gb, R.AL * c["dy"], (R.AL * c["dy"]).abs(), mode, "ops.axpby d b")
    dot, S = R.dot_ref(c["dy"], c["b"])
    depth = max(R.stride_geom(n // 8, 2048)["depth"], R.stride_geom(n // 8, 512)["depth"])
    check_red(gal, [dot], [S], depth, 1, "ops.axpby d alpha")


# ------------------------------------------------------------------------------------------ colsum
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("case", list(R.COLSUM_CASES))
def test_colsum(case, mode):
    dt, code, st = setup(mode)
    rows, Cc = case
    x = R.randn(R.gen_for("colsum", case, mode), (rows, Cc), mode, device=DEV)
    xd = dev(x, mode)
    g = R.colsum_geom(rows, Cc)
    ref, S = x.sum(0), x.abs().sum(0)
    out = torch.zeros(Cc, dtype=torch.float32, device=DEV)
    L.call("xmc_colsum", p(xd), p(out), rows, Cc, code, st)
    check_red(out, ref, S, g["depth"], 0, f"colsum {case} {mode}")
    pre = torch.randn(Cc, generator=R.gen_for("colsum-pre", case)).to(DEV)
    out = pre.clone()
    L.call("xmc_colsum", p(xd), p(out), rows, Cc, code, st)
    check_red(out, ref + pre.double(), S + pre.double().abs(), g["depth"], 0, f"colsum += {case} {mode}")


# ------------------------------------------------------------------------------------------ pool / upsample / axpby_up / axpby_bwd / gap
def check_axpby_bwd(c, d, lo, mode, up, masked, want_db):
    N, H, W, Cc = lo
    al = torch.tensor([R.AL], dtype=torch.float32, device=DEV)
    da, db, dal = ops._axpby_bwd_fused(d["dy"], d["b"], al, up, ymask=d["ymask"] if masked else None, want_db=want_db)
    rda, A_da, rdb, A_db, rdal, S = R.axpby_bwd_ref(c["dy"], c["b"], R.AL, up, c["ymask"] if masked else None)
    what = f"axpby_bwd {lo} {mode} up={up} ymask={masked} want_db={want_db}"
    assert (db is None) == (not want_db) and (da is None) == (rda is None), what
    if want_db:
        check_elem(db, rdb, A_db, mode, what + " db")
    if rda is not None:
        check_elem(da, rda, A_da, mode, what + " da")
    total = N * H * W * Cc // 8 * (1 if up else 4)
    check_red(dal, [rdal], [S], R.stride_geom(total, 2048, 32 if up else 8)["depth"], 3, what + " dalpha")


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("lo", [R.RESAMPLE_SMALL, R.RESAMPLE_BIG])
def test_pool_upsample_axpby_gap(lo, mode):
    dt, code, st = setup(mode)
    N, H, W, Cc = lo
    c = R.resample_case(lo, mode, device=DEV if lo == R.RESAMPLE_BIG else None)
    d = {k: dev(v, mode) for k, v in c.items()}
    al = torch.tensor([R.AL], dtype=torch.float32, device=DEV)
    check_elem(ops.avgpool2(d["dy"]), *R.sumpool2_ref(c["dy"], 0.25), mode, f"avgpool2 {lo} {mode}")
    for scale in (1.0, 0.25):
        out = torch.empty((N, H, W, Cc), dtype=dt, device=DEV)
        L.call("xmc_sumpool2", p(d["dy"]), p(out), N, 2 * H, 2 * W, Cc, scale, code, st)
        check_elem(out, *R.sumpool2_ref(c["dy"], scale), mode, f"sumpool2 x{scale} {lo} {mode}")
    check_exact(ops.upsample2(d["a"]), R.up2_ref(c["a"]), f"upsample2 {lo} {mode}")
    for lrelu in (False, True):
        check_elem(ops.axpby_up(d["a"], d["b"], al, lrelu), *R.axpby_up_ref(c["a"], c["b"], R.AL, lrelu), mode, f"axpby_up lrelu={lrelu} {lo} {mode}")
    for up in (False, True):
        for masked in (False, True):
            for want_db in (True, False):
                check_axpby_bwd(c, d, lo, mode, up, masked, want_db)
    # global average pool (both branches of the launcher between the two shapes) and its backward on the high-resolution map
    g = R.gap_geom(N, H * W, Cc)
    ref, S = R.gap_ref(c["a"])
    check_red(ops.global_avgpool(d["a"]), ref, S, g["depth"], 2, f"global_avgpool ({g['branch']}) {lo} {mode}")
    w = R.rand_f32(R.gen_for("gap-bwd", lo), (N, Cc), device=c["a"].device)
    dx, wd = torch.empty((N, 2 * H, 2 * W, Cc), dtype=dt, device=DEV), dev(w)
    L.call("xmc_global_avgpool_bwd", p(wd), p(dx), N, 4 * H * W, Cc, code, L.F32, st)
    check_elem(dx, *R.gap_bwd_ref(w, 2 * H, 2 * W), mode, f"global_avgpool_bwd {lo} {mode}")


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_global_avgpool_bwd_is_exact_when_the_divisor_is_a_power_of_two(mode):
    dt, code, st = setup(mode)
    N, H, W, Cc = 2, 4, 8, 24
    w = R.randn(R.gen_for("gap-exact"), (N, Cc), mode)
    dx, wd = torch.empty((N, H, W, Cc), dtype=dt, device=DEV), dev(w)
    L.call("xmc_global_avgpool_bwd", p(wd), p(dx), N, H * W, Cc, code, L.F32, st)
    check_exact(dx, R.gap_bwd_ref(w, H, W)[0].contiguous(), "global_avgpool_bwd 1/32")
    y = ops.global_avgpool(dev(R.up2_ref(w[:, None, None, :].expand(N, 2, 4, Cc).contiguous()), mode))
    check_red(y, w, w.abs(), R.gap_geom(N, H * W, Cc)["depth"], 2, "global_avgpool of a constant map")


def test_pool2_second_lap():
    dt, code, st = setup("bf16")
    N, H, W, Cc = R.RESAMPLE_BIG2
    x = R.randn(R.gen_for("pool2-big"), (N, 2 * H, 2 * W, Cc), "bf16", device=DEV)
    check_elem(ops.avgpool2(dev(x, "bf16")), *R.sumpool2_ref(x, 0.25), "bf16", f"avgpool2 -> {R.RESAMPLE_BIG2}")


def test_axpby_bwd_up_second_lap():
    setup("bf16")
    c = R.resample_case(R.RESAMPLE_UPBWD, "bf16", want=("b", "dy", "ymask"), device=DEV)
    d = {k: dev(v, "bf16") for k, v in c.items()}
    check_axpby_bwd(c, d, R.RESAMPLE_UPBWD, "bf16", True, True, True)


# ------------------------------------------------------------------------------------------ NCHW f32 <-> NHWC8
@pytest.mark.parametrize("shape,mode", [(s, m) for s in R.CONVERT_SMALL for m in R.MODES] + [(R.CONVERT_BIG, "bf16")])
def test_layout_converters_are_bit_exact(shape, mode):
    dt, code, st = setup(mode)
    N, Cc, H, W = shape
    img = (torch.rand(shape, generator=R.gen_for("img", shape)) * 2 - 1).to(DEV)
    z = ops.to_nhwc8(img)
    assert z.shape == (N, H, W, 8) and z.dtype == dt
    want = img.to(dt).permute(0, 2, 3, 1)
    assert torch.equal(z[..., :Cc], want), "to_nhwc8: values"
    assert Cc == 8 or float(z[..., Cc:].float().abs().max()) == 0.0, "to_nhwc8: padding channels"
    back = ops.to_nchw(z, Cc)
    assert back.dtype == torch.float32 and torch.equal(back, img.to(dt).float()), "to_nchw"
    # the other way round from a tensor whose padding channels are NOT zero: they must not leak into the image
    z2 = z.clone()
    z2[..., Cc:] = 3.0
    assert torch.equal(ops.to_nchw(z2, Cc), back)


# ------------------------------------------------------------------------------------------ hinge
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("n", R.HINGE_N)
def test_hinge(n, mode):
    dt, code, st = setup(mode)
    v = R.hinge_case(n, mode)
    pad = R.randn(R.gen_for("hinge-pad", n), (n, 1, 1, 8), mode)
    pad[:, 0, 0, 0] = v
    for sign in (-1.0, 1.0):
        loss, S, grad = R.hinge_ref(v, sign)
        lgd = dev(pad, mode).requires_grad_()
        out = ops.hinge(lgd[..., :1].permute(0, 3, 1, 2), sign)           # the stride-8 view the discriminator hands over
        check_red(out, [loss], [S], R.hinge_depth(n), 2, f"hinge n={n} sign={sign} {mode}")
        out.backward()
        check_elem(lgd.grad[:, 0, 0, 0], grad, grad.abs(), mode, f"hinge gradient n={n} sign={sign} {mode}")
        assert float(lgd.grad[..., 1:].float().abs().max()) == 0.0
        # the kernels themselves on the padded tensor, stride 8
        x = dev(pad, mode)
        o = torch.empty(1, dtype=torch.float32, device=DEV)
        L.call("xmc_hinge_fwd", p(x), 8, sign, p(o), n, code, st)
        check_red(o, [loss], [S], R.hinge_depth(n), 2, f"xmc_hinge_fwd stride 8 n={n} {mode}")
        dx, one = torch.zeros_like(x), torch.ones(1, device=DEV)
        L.call("xmc_hinge_bwd", p(x), 8, sign, p(one), p(dx), n, code, st)
        check_elem(dx[:, 0, 0, 0], grad, grad.abs(), mode, f"xmc_hinge_bwd stride 8 n={n} {mode}")
        assert float(dx[..., 1:].float().abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ the DF-GAN affine pair
def check_affine_bwd(shape, mode, two, with_dx_in, with_alpha, pool, rdev=None, inputs=None):
    N, H, W, Cc = shape
    x, ps, dy, dx_in = inputs or R.affine_case(shape, mode, two, device=rdev)
    alpha = 0.625 if with_alpha else None
    ref = R.affine_ref(x, ps, mode, dy, dx_in if with_dx_in else None, alpha, pool)
    g = R.affine_bwd_geom(N, H, W, Cc, pool)
    what = f"affine bwd {shape} {mode} two={two} dx_in={with_dx_in} alpha={with_alpha} pool={pool}"
    dot = torch.full((1,), PREFILL, dtype=torch.float32, device=DEV) if with_alpha else None
    al = torch.tensor([alpha], dtype=torch.float32, device=DEV) if with_alpha else None
    res = ops._affine_bwd_raw(dev(x, mode), dev(dy, mode), [dev(t) for t in ps], 0.2, dx_acc=dev(dx_in, mode) if with_dx_in else None,
                              alpha=al, dot=dot, want_sumpool=pool)
    check_elem(res[0], ref["dx"], ref["A_dx"], mode, what + " dx")
    assert res[1].shape == (len(ps), N, Cc)
    for i, (val, S) in enumerate(ref["grads"]):
        check_red(res[1][i], val, S, g["depth_param"], R.AFFINE_GRAD_OPS, what + " " + ("dg0", "db0", "dg1", "db1")[i])
    if with_alpha:
        check_red(dot, [PREFILL + ref["dot"]], [PREFILL + ref["S_dot"]], g["depth_dot"], 1, what + " dot", ref["slack_dot"])
    if pool:
        err = (f64(res[2], ref["pool"]) - ref["pool"]).abs()
        bound = R.elem_bound(ref["pool"], ref["A_pool"], mode) + ref["slack_pool"]
        assert bool((err <= bound).all()), f"{what} pooled dx: {int((err > bound).sum())} beyond the bound, worst ratio {float((err / bound).max()):.3f}"


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", list(R.AFFINE_CASES) + list(R.AFFINE_POOL_CASES))
def test_affine_forward(shape, mode):
    setup(mode)
    for two in (True, False):
        x, ps, _, _ = R.affine_case(shape, mode, two)
        ref = R.affine_ref(x, ps, mode)
        y = ops._affine_fwd_raw(dev(x, mode), [dev(t) for t in ps], 0.2)
        check_elem(y, ref["y"], ref["A_y"], mode, f"affine fwd {shape} {mode} two={two}")


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", list(R.AFFINE_CASES))
def test_affine_backward(shape, mode):
    setup(mode)
    combos = [(True, False, False), (False, False, False), (True, True, False), (True, False, True)]
    if shape in R.AFFINE_CROSS:
        combos = [(t, d, a) for t in (True, False) for d in (False, True) for a in (False, True)]
    for two, with_dx_in, with_alpha in combos:
        check_affine_bwd(shape, mode, two, with_dx_in, with_alpha, False)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", list(R.AFFINE_POOL_CASES))
def test_affine_backward_pooled(shape, mode):
    setup(mode)
    combos = [(True, False, False)]
    if shape in R.AFFINE_POOL_CROSS:
        combos = [(t, d, a) for t in (True, False) for d in (False, True) for a in (False, True)]
    for two, with_dx_in, with_alpha in combos:
        check_affine_bwd(shape, mode, two, with_dx_in, with_alpha, True)


def test_affine_backward_large():
    """33M elements: ppl = 64 with several pixel blocks per image and a partial last one; dx_in + dot"""
    setup("bf16")
    check_affine_bwd(R.AFFINE_BIG, "bf16", True, True, True, False, rdev=DEV)


@pytest.mark.parametrize("mode", R.MODES)
def test_affine_pool_refused_shapes_write_nothing(mode):
    dt, code, st = setup(mode)
    for N, H, W, Cc in R.AFFINE_POOL_REFUSED:
        x = torch.zeros((N, H, W, Cc), dtype=dt, device=DEV)
        ps = [torch.ones((N, Cc), device=DEV) for _ in range(4)]
        dx = torch.full_like(x, SENT)
        red = torch.full((4, N, Cc), SENT, device=DEV)
        dxp = torch.full((N, max(H // 2, 1), max(W // 2, 1), Cc), SENT, dtype=dt, device=DEV)
        rc = L.load().xmc_affine2_act_bwd(p(x), p(x), *[p(t) for t in ps], p(dx), *[p(red[i]) for i in range(4)], None, None, None,
                                          p(dxp), N, H, W, Cc, 0.2, code, st)
        torch.cuda.synchronize()
        assert rc == -3, ((N, H, W, Cc), rc)                      # XMC_ESHAPE
        assert bool((dx == SENT).all()) and bool((red == SENT).all()) and bool((dxp == SENT).all()), (N, H, W, Cc)


@pytest.mark.parametrize("mode", R.MODES)
def test_affine_wrappers_through_autograd(mode):
    """ops.affine2_lrelu / affine_lrelu / affine_act (ReLU) / affine2_lrelu_skip on the anchor case: same kernels, reached through autograd"""
    setup(mode)
    shape = (3, 6, 6, 24)
    N, H, W, Cc = shape
    g = R.affine_bwd_geom(*shape)

    def run(fn, two, slope, skip=False):
        x, ps, dy, dx_in = R.affine_case(shape, mode, two, slope)
        ref = R.affine_ref(x, ps, mode, dy, dx_in if skip else None, slope=slope)
        xd = dev(x, mode).requires_grad_()
        pd = [dev(t).requires_grad_() for t in ps]
        out = fn(xd, *pd)
        y, loss = (out[0], (out[0].float() * dev(dy)).sum() + (out[1].float() * dev(dx_in)).sum()) if skip else (out, (out.float() * dev(dy)).sum())
        check_elem(y, ref["y"], ref["A_y"], mode, f"{fn.__name__} {mode} y")
        grads = torch.autograd.grad(loss, [xd] + pd)
        check_elem(grads[0], ref["dx"], ref["A_dx"], mode, f"{fn.__name__} {mode} dx")
        for got, (val, S) in zip(grads[1:], ref["grads"]):
            check_red(got, val, S, g["depth_param"], R.AFFINE_GRAD_OPS, f"{fn.__name__} {mode} parameter gradient")

    run(ops.affine2_lrelu, True, R.SLOPE)
    run(ops.affine_lrelu, False, R.SLOPE)
    run(lambda x, g0, b0: ops.affine_act(x, g0, b0, 0.0), False, 0.0)
    run(ops.affine2_lrelu_skip, True, R.SLOPE, skip=True)
