"""tests/pointwise_ref.py checked without a GPU: the closed-form gradients against f64 autograd, every case's regime predicate against
the model of the launch geometry, and the "no pre-activation within 1e-3 of a LeakyReLU kink" condition of every case that has one."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointwise_ref as R


def close(a, b, tol=1e-12):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * (1 + float(b.abs().max())), float((a - b).abs().max())


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------ closed forms against autograd
@pytest.mark.parametrize("two", [True, False])
@pytest.mark.parametrize("with_dx_in", [False, True])
@pytest.mark.parametrize("with_alpha", [False, True])
@pytest.mark.parametrize("slope", [R.SLOPE, 0.0])
def test_affine_closed_forms(two, with_dx_in, with_alpha, slope):
    shape, mode = (2, 4, 6, 8), "fp32"
    x, ps, dy, dx_in = R.affine_case(shape, mode, two, slope)
    al = 0.625 if with_alpha else None
    ref = R.affine_ref(x, ps, mode, dy, dx_in if with_dx_in else None, al, pool=True, slope=slope)
    xa = x.clone().requires_grad_()
    pa = [p.clone().requires_grad_() for p in ps]
    e = lambda t: t[:, None, None, :]
    y = F.leaky_relu(xa * e(pa[0]) + e(pa[1]), slope)
    if two:
        y = F.leaky_relu(y * e(pa[2]) + e(pa[3]), slope)
    close(ref["y"], y.detach())
    assert bool((ref["A_y"] >= ref["y"].abs() * (1 - 1e-12)).all())
    loss = ((al if with_alpha else 1.0) * y * dy).sum() + ((xa * dx_in).sum() if with_dx_in else 0.0)
    grads = torch.autograd.grad(loss, [xa] + pa)
    close(ref["dx"], grads[0])
    assert len(ref["grads"]) == len(ps)
    for (val, S), want in zip(ref["grads"], grads[1:]):
        close(val, want)
        assert bool((S >= val.abs() * (1 - 1e-12)).all())
    if with_alpha:
        # d/d alpha of <dy, alpha y> with the y the consumer read: the rounded one (fp32: f32 rounding of the f64 value)
        close(ref["dot"], float((dy * R.rt(y.detach(), mode)).sum()))
        assert ref["S_dot"] >= abs(ref["dot"]) and ref["slack_dot"] >= 0
    close(ref["pool"], nhwc(F.avg_pool2d(nchw(R.rt(ref["dx"], mode)), 2) * 4))
    assert ref["pool"].shape == (2, 2, 3, 8)


def test_affine_rounded_dot_and_pool_use_the_storage_format():
    """bf16: dot is taken against round(y) and the pool over round(dx), and the flip slack is zero except next to a rounding boundary"""
    x, ps, dy, _ = R.affine_case((2, 4, 6, 8), "bf16")
    ref = R.affine_ref(x, ps, "bf16", dy, None, 0.5, pool=True)
    assert abs(ref["dot"] - float((dy * ref["y"]).sum())) > 0           # rounding y matters in bf16
    assert ref["slack_dot"] <= 2.0 ** -7 * ref["S_dot"]
    assert float(ref["slack_pool"].max()) <= 2.0 ** -6 * float(ref["A_pool"].max())
    assert float((ref["slack_pool"] == 0).double().mean()) > 0.9


@pytest.mark.parametrize("up", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_axpby_closed_forms(up, masked):
    mode = "fp32"
    c = R.resample_case((2, 3, 5, 8), mode)
    a_lo, b, dy, al = c["a"], c["b"], c["dy"], R.AL
    if not up:
        a_lo = R.resample_case((2, 6, 10, 8), mode, want=("a",))["a"]
        b = R.fix_kinks(b, lambda t: (a_lo + al * t,), mode)
    aa, ba, ala = a_lo.clone().requires_grad_(), b.clone().requires_grad_(), torch.tensor(al, dtype=torch.float64, requires_grad=True)
    a_hi = nhwc(F.interpolate(nchw(aa), scale_factor=2)) if up else aa
    if up:
        close(R.up2_ref(a_lo), a_hi.detach())
    y = a_hi + ala * ba
    pre = y.detach()               # the mask only reads the sign, which LeakyReLU keeps: the pre-activation stands in for the stored y
    yref, A = (R.axpby_up_ref(a_lo, b, al, masked) if up else R.axpby_ref(a_lo, b, al))
    if masked:
        y = F.leaky_relu(y, R.SLOPE)
        if not up:
            yref, A = R.lrelu_ref(yref)
    close(yref, y.detach())
    ga, gb, gal = torch.autograd.grad((y * dy).sum(), [aa, ba, ala])
    da, A_da, db, A_db, dal, S = R.axpby_bwd_ref(dy, b, al, up, pre if masked else None)
    close(db, gb)
    close(dal, gal)
    assert S >= abs(dal)
    if da is None:
        close(dy, ga)              # plain form without a mask: da is dy itself, the kernel writes none
    else:
        close(da, ga)


def test_flat_closed_forms():
    c = R.flat_case(64, "fp32")
    x = c["x"].clone().requires_grad_()
    y = F.leaky_relu(x, R.SLOPE)
    close(R.lrelu_ref(c["x"])[0], y.detach())
    close(R.mask_ref(c["dy"], c["x"])[0], torch.autograd.grad((y * c["dy"]).sum(), x)[0])
    x = c["b"].clone().requires_grad_()
    t = torch.tanh(x)
    close(R.tanh_bwd_ref(c["dy"], t.detach())[0], torch.autograd.grad((t * c["dy"]).sum(), x)[0])
    # scale_mask_dot: the backward of s + alpha * lrelu(r) towards r and alpha, `ref` being lrelu's OUTPUT (same sign as its input)
    r, al = c["ref"].clone().requires_grad_(), torch.tensor(R.AL, dtype=torch.float64, requires_grad=True)
    out = F.leaky_relu(r, R.SLOPE)
    gr, gal = torch.autograd.grad((al * out * c["dy"]).sum(), [r, al])
    g, A, dot, S = R.scale_mask_dot_ref(c["dy"], out.detach(), R.AL)
    close(g, gr)
    close(dot, gal)
    assert S >= abs(dot) and bool((A >= g.abs()).all())


def test_pool_gap_hinge_closed_forms():
    c = R.resample_case((2, 3, 5, 8), "fp32", want=("a", "dy"))
    x = c["dy"].clone().requires_grad_()
    p = nhwc(F.avg_pool2d(nchw(x), 2))
    close(R.sumpool2_ref(c["dy"], 0.25)[0], p.detach())
    close(R.sumpool2_ref(c["dy"], 1.0)[0], 4 * p.detach())
    # up2 (scale 1) is the adjoint of the 2x2 sum pool
    close(R.up2_ref(c["a"]), torch.autograd.grad((4 * p * c["a"]).sum(), x)[0])
    g = nhwc(F.adaptive_avg_pool2d(nchw(x), 1)).reshape(2, 8)
    close(R.gap_ref(c["dy"])[0], g.detach())
    w = c["a"][:, 0, 0, :]
    close(R.gap_bwd_ref(w, 6, 10)[0], torch.autograd.grad((g * w).sum(), x)[0])
    for sign in (-1.0, 1.0):
        v = R.kinkfree(R.gen_for("hinge", sign), (9,), "fp32").clone().requires_grad_()
        loss = F.relu(1 + sign * v).mean()
        want, S, grad = R.hinge_ref(v.detach(), sign)
        close(want, loss.detach())
        close(grad, torch.autograd.grad(loss, v)[0])


# ------------------------------------------------------------------------------------------ the model of the launch geometry
def test_geometry_model_constants_match_the_source():
    """the constants restated in pointwise_ref.py are those of csrc/pointwise.hip (a retuned launcher must be restated there too)"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "xmc-gan_amd", "csrc", "pointwise.hip")).read()
    for text in ("constexpr int NT = 256;", "constexpr int UN = 4;", "constexpr int STREAM_BLOCKS = 1024;", "int cap = 256 * 16",
                 "nblocks(n8, NT, 512)", "nblocks(rows, groups * 8, 1024)", "nblocks(total, NT, 2048)", "affine_grid(HW, C / 8, N, g, ppb, 16)",
                 "affine_grid(HW, C / 8, N, g, ppb, dx_pool ? 32 : 64)", "while (ppl > 4 && (long long)N * ((HW + groups * ppl - 1) / (groups * ppl)) < 256) ppl >>= 1;",
                 "if (HW >= 256 && out_dtype == XMC_F32 && C / 8 <= NT", "((int64_t)N * HW + 2047) / 2048", "if (ppb < 4 * groups) ppb = 4 * groups;"):
        assert text in src, text


def test_geometry_model_by_hand():
    assert R.nblocks(0) == 1 and R.nblocks(257) == 2 and R.nblocks(10 ** 9) == 4096
    assert R.sblocks(1) == 1 and R.sblocks(1024) == 1 and R.sblocks(1025) == 2 and R.sblocks(10 ** 8) == 1024
    # 64 images of 32x32 with 64 channels (the comment in affine_grid): 32 pixel lanes, ppl 64 -> 8 (64 * 4 = 256 workgroups)
    assert R.affine_grid(1024, 8, 64, 64) == dict(groups=32, ppl=8, bx=4, ppb=256)
    assert R.affine_grid(1024, 8, 512, 64) == dict(groups=32, ppl=64, bx=1, ppb=1024)
    g = R.colsum_geom(64, 2056)
    assert (g["gx"], g["gy"], g["groups_host"]) == (8, 2, 1) and [y["groups"] for y in g["ys"]] == [1, 256]
    assert R.gap_geom(2, 16, 64)["branch"] == "small" and R.gap_geom(2, 256, 64, out_f32=False)["branch"] == "small"
    assert R.gap_geom(64, 128 * 128, 128) == dict(branch="big", groups=16, ppb=512, bx=32, depth=32 + 16 + 32)


@pytest.mark.parametrize("n", list(R.FLAT_REGIMES))
def test_flat_case_regimes(n):
    what, pred = R.FLAT_REGIMES[n]
    assert n % 8 == 0 and pred(n // 8), what


@pytest.mark.parametrize("case", list(R.COLSUM_CASES))
def test_colsum_case_regimes(case):
    what, pred = R.COLSUM_CASES[case]
    assert pred(R.colsum_geom(*case)), what


def test_resample_and_convert_case_regimes():
    for what, ok in R.resample_regimes():
        assert ok, what
    N, C, H, W = R.CONVERT_BIG
    assert R.stride_geom(N * H * W)["laps"] == 2 and [c[1] for c in R.CONVERT_SMALL] == list(range(1, 9))
    assert [R.hinge_depth(n) for n in R.HINGE_N] == [11, 11, 11, 12, 14]       # one lap, and more than one, of the single workgroup


@pytest.mark.parametrize("case", list(R.AFFINE_CASES) + [R.AFFINE_BIG])
def test_affine_case_regimes(case):
    what, pred = R.AFFINE_CASES.get(case, R.AFFINE_BIG_REGIME)
    assert pred(R.affine_bwd_geom(*case)), (what, R.affine_bwd_geom(*case))


def test_affine_cases_cover_every_regime_between_them():
    gs = [R.affine_bwd_geom(*c) for c in R.AFFINE_CASES]
    assert {g["ppl"] for g in gs} >= {4, 64} and {g["C8"] for g in gs} >= {1, 3, 8, R.NT}
    assert any(g["bx"] > 1 for g in gs) and any(g["steps_with_second"] and g["steps_without_second"] for g in gs)
    assert all(c in R.AFFINE_CASES for c in R.AFFINE_CROSS) and all(c in R.AFFINE_POOL_CASES for c in R.AFFINE_POOL_CROSS)


@pytest.mark.parametrize("case", list(R.AFFINE_POOL_CASES))
def test_affine_pool_case_regimes(case):
    what, pred = R.AFFINE_POOL_CASES[case]
    N, H, W, C = case
    g = R.affine_bwd_geom(*case, pool=True)
    assert H % 2 == 0 and W % 2 == 0 and g["C8"] in (1, 2, 4, 8, 16, 32) and g["ppb"] % 2 == 0 and g["groups"] % 2 == 0
    assert pred(g), (what, g)


def test_affine_pool_cases_cover_every_lane_distance_and_both_parities():
    assert {c[3] // 8 for c in R.AFFINE_POOL_CASES} == {1, 2, 4, 8, 16, 32}
    assert {(c[2] // 2) % 2 for c in R.AFFINE_POOL_CASES} == {0, 1}
    for N, H, W, C in R.AFFINE_POOL_REFUSED:
        assert H % 2 or W % 2 or (C // 8) & (C // 8 - 1) or C // 8 > 32


# ------------------------------------------------------------------------------------------ no element within 1e-3 of a kink
@pytest.mark.parametrize("mode", R.MODES)
def test_small_cases_are_kink_free(mode):
    for n in R.FLAT_SMALL:
        c = R.flat_case(n, mode)
        assert R.min_abs(c["x"], c["ref"]) >= R.KINK
    c = R.resample_case(R.RESAMPLE_SMALL, mode)
    assert R.min_abs(c["ymask"], R.up2_ref(c["a"]) + R.AL * c["b"]) >= R.KINK
    for two in (True, False):
        for case in list(R.AFFINE_CASES) + list(R.AFFINE_POOL_CASES):
            x, ps, _, _ = R.affine_case(case, mode, two)
            assert R.affine_ref(x, ps, mode)["kink"] >= R.KINK, case
    for n in R.HINGE_N:
        assert float((1 - R.hinge_case(n, mode).abs()).abs().min()) >= R.KINK


def test_large_cases_are_kink_free():
    c = R.flat_case(R.FLAT_BIG, "bf16")
    assert R.min_abs(c["x"], c["ref"]) >= R.KINK
    for lo in (R.RESAMPLE_BIG, R.RESAMPLE_UPBWD):
        c = R.resample_case(lo, "bf16", want=("a", "b", "ymask"))
        assert R.min_abs(c["ymask"], R.up2_ref(c["a"]) + R.AL * c["b"]) >= R.KINK
    x, ps, _, _ = R.affine_case(R.AFFINE_BIG, "bf16")
    assert R.affine_ref(x, ps, "bf16")["kink"] >= R.KINK
