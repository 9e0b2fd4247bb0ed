"""The convolution weight-gradient kernels, bit for bit, on every branch of their dispatch (the case tables of tests/wgrad_ref.py;
tests/test_wgrad_cpu.py holds every case to the kernel and the regime it names on the model).

Everything goes through ops._conv_wgrad_raw, the entry of every autograd node.  Each test first asserts that the kernel that ran
(xmc_last_kernel) is the one the model predicts.  Class I (dense integers in [-3, 3]) and class II (one operand zero except at one
pixel the model singles out: corners, tile seams, split seams, a K step that starts mid-image, the last pixel) have exact f32 results
whatever the order of the additions, and are compared with torch.equal against the f64 reference cast to f32.  Class III (dense
Gaussian, one case per kernel family and mode) is held to |got - ref| <= P 2^-23 sum|x dy| per element; the largest err / bound
measured on the MI355X is 4.4e-4 (fp32), 5.3e-4 (bf16), 4.7e-4 (f16).

What the classes are each there for, from arithmetic-only, in-bounds mutations of a scratch copy of one kernel file (never
committed), against these tests / against test_conv_fwd_dgrad_wgrad, test_upsample_conv_fusion and
test_upsample_wgrad_low_resolution_kernel of test_ops_gpu.py:
  1  split-K: x side reads `p + 1 < p_end` (last pixel of a split zero)        I, II, III fail / noticed (fp32 cases mostly)
  2  split-K: right border `sw < SWv - 1`                                      I, II, III fail / noticed
  3  row: right halo column of a K step's last segment staged as zero          I, II fail, on the 4x128 case alone (the one map
                                                                               where that column lies inside the image) / not noticed
  4  row-reuse tile: bottom halo of the bottom tile row read from the last row I, II, III fail / noticed
  5  split-K: bias sum skips the workgroup with the largest blockIdx.x         I, II, III fail (db) / noticed
  6  up: class -> tap entries (cp, u) = (0, 0) and (1, 1) swapped              I, II, III fail / noticed
  7  split-K: low three mantissa bits of x cleared while staged                I passes; II fails in all three modes; III fails in
                                                                               bf16 and f16, passes in fp32 / not noticed
Mutation 7 is why class II exists: integers in [-3, 3] have no low mantissa bits to lose."""
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_ref as R

if torch.cuda.is_available():
    from xmc_gan_amd import lib as L
    from xmc_gan_amd import ops

DEV = "cuda"
RUNS = R.all_runs()
RUN_IDS = [f"{t}-{R.case_id(e.case)}-{mode}" for t, e, mode in RUNS]
RUNS3 = [(e, mode) for e, modes in R.CLASS3 for mode in modes]
RUN3_IDS = [f"{R.case_id(e.case)}-{mode}" for e, mode in RUNS3]


@pytest.fixture(autouse=True)
def _restore_precision():
    yield
    ops.set_precision("bf16")


def to_nhwc(t, cpad, mode):
    """NCHW f64 on the host (values the format holds exactly) -> NHWC, padded with zero channels, in the format, on the device"""
    N, Cc, H, W = t.shape
    y = torch.zeros(N, H, W, cpad, dtype=R.DTYPE[mode])
    y[..., :Cc] = t.permute(0, 2, 3, 1).to(R.DTYPE[mode])
    return y.to(DEV).contiguous()


def launch(c, mode, xd, dyd):
    """-> (dW [cout, cin / g, k, k] f32, db [CD] f32 or None, the kernel that ran)"""
    geom = ops.ConvGeom(c.cin, c.cout, c.k, c.s, c.p, groups=c.groups)
    ops.new_iteration(DEV)
    r = ops._conv_wgrad_raw(xd, dyd, geom, up=c.up, want_bias=R.want_bias(c))
    kernel = L.load().xmc_last_kernel().decode()
    gw, gb = r if R.want_bias(c) else (r, None)
    return gw.cpu(), (None if gb is None else gb.cpu()), kernel


def begin(e, mode):
    ops.set_precision(mode)
    assert ops.act_dtype() == R.DTYPE[mode]
    c = e.case
    d = R.desc(c, mode)
    assert ops.chan_pad(c.cin, ops.act_dtype()) == d.CS and ops.pad_to(c.cout, 8) == d.CD
    return c, d, R.predict_kernel(c, mode)


@functools.lru_cache(maxsize=None)
def ints_ref(c):
    """class I operands and their reference: the same in every mode"""
    x, dy = R.ints(c)
    dW, db = R.wgrad_ref(x, dy, c.k, c.s, c.p, c.up, c.groups)
    return x, dy, dW.float(), db.float()


def first_difference(got, exp):
    """message: taps that differ and the first differing (co, ci) of the first of them"""
    bad = (got != exp)
    taps = [(int(kh), int(kw)) for kh, kw in bad.any(dim=0).any(dim=0).nonzero()]
    kh, kw = taps[0]
    co, ci = (int(v) for v in bad[:, :, kh, kw].nonzero()[0])
    return (f"{int(bad.sum())} of {bad.numel()} elements differ, in taps {taps}; first in tap ({kh}, {kw}) at (co, ci) = ({co}, {ci}): "
            f"got {float(got[co, ci, kh, kw])!r}, expected {float(exp[co, ci, kh, kw])!r}")


def check_dw(got, exp, what):
    assert got.dtype == torch.float32 and got.shape == exp.shape, (what, got.shape, exp.shape)
    if not torch.equal(got, exp):
        raise AssertionError(f"{what}: dW is not bit-exact: " + first_difference(got, exp))


def check_db(gb, exp, c, d, what):
    assert gb.dtype == torch.float32 and gb.shape == (d.CD,), (what, gb.shape)
    bad = (gb[:c.cout] != exp).nonzero().flatten().tolist()
    assert not bad, f"{what}: db is not bit-exact at channels {bad[:8]}: got {gb[bad[:8]].tolist()}, expected {exp[bad[:8]].tolist()}"
    assert not gb[c.cout:].any(), f"{what}: the padded bias rows are not zero: {gb[c.cout:].tolist()}"


# ------------------------------------------------------------------------------------------ class I
@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
def test_dense_integers_bit_exact(run):
    _, e, mode = run
    c, d, want = begin(e, mode)
    x, dy, dW, db = ints_ref(c)
    gw, gb, kernel = launch(c, mode, to_nhwc(x, d.CS, mode), to_nhwc(dy, d.CD, mode))
    assert kernel == want, f"the model predicts {want}, {kernel} ran ({e.why})"
    assert gw.shape == (c.cout, c.cin // c.groups, c.k, c.k)          # the padded rows co >= cout stay behind
    check_dw(gw, dW, "class I")
    if gb is not None:
        check_db(gb, db, c, d, "class I")


# ------------------------------------------------------------------------------------------ class II
@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
def test_single_pixel_impulses_bit_exact(run):
    _, e, mode = run
    c, d, want = begin(e, mode)
    x, dy = R.gauss(c, mode)
    xd, dyd = to_nhwc(x, d.CS, mode), to_nhwc(dy, d.CD, mode)
    zx, zdy = torch.zeros_like(xd), torch.zeros_like(dyd)

    def probe(which, name, n, i, j):
        v = R.impulse_values(c, mode, which, name)
        dense, hole = (dy, zx) if which == "x" else (x, zdy)
        hole[n, i, j, :v.numel()] = v.to(R.DTYPE[mode]).to(DEV)
        gw, gb, kernel = launch(c, mode, *((hole, dyd) if which == "x" else (xd, hole)))
        hole[n, i, j].zero_()
        assert kernel == want, f"the model predicts {want}, {kernel} ran ({e.why})"
        # the reference needs image n only: every other image of the impulse operand is zero
        imp = torch.zeros_like((x if which == "x" else dy)[n:n + 1])
        imp[0, :, i, j] = v
        dW, db = R.wgrad_ref(*((imp, dense[n:n + 1]) if which == "x" else (dense[n:n + 1], imp)), c.k, c.s, c.p, c.up, c.groups)
        what = f"class II, {which}-impulse '{name}' at (n, row, col) = ({n}, {i}, {j})"
        check_dw(gw, dW.float(), what)
        if gb is not None and which == "dy":
            assert torch.equal(db.float(), v.float())
            check_db(gb, v.float(), c, d, what)          # db is the impulse itself

    for name, (n, a, b) in R.probes(c, mode).items():
        probe("dy", name, n, a, b)
    if not c.up:          # through the upsample a source pixel feeds up to four outputs per tap: not a single product
        for name, (n, i, j) in R.x_probes(c, mode).items():
            probe("x", name, n, i, j)


# ------------------------------------------------------------------------------------------ class III
@pytest.mark.parametrize("run", RUNS3, ids=RUN3_IDS)
def test_dense_gaussian_within_the_summation_bound(run):
    e, mode = run
    c, d, want = begin(e, mode)
    x, dy = R.gauss(c, mode)
    gw, gb, kernel = launch(c, mode, to_nhwc(x, d.CS, mode), to_nhwc(dy, d.CD, mode))
    assert kernel == want, f"the model predicts {want}, {kernel} ran ({e.why})"
    dW, db = R.wgrad_ref(x, dy, c.k, c.s, c.p, c.up, c.groups)
    bW, bb = R.class3_bound(x, dy, c)
    rW = float(((gw.double() - dW).abs() / bW.clamp_min(1e-300)).max())
    rb = float(((gb[:c.cout].double() - db).abs() / bb.clamp_min(1e-300)).max())
    print(f"class III {R.case_id(c)} {mode} {kernel}: worst err / bound = {rW:.3e} (dW), {rb:.3e} (db)")
    assert rW <= 1.0, f"dW: {int(((gw.double() - dW).abs() > bW).sum())} of {dW.numel()} elements beyond P 2^-23 sum|x dy|, worst ratio {rW:.3f}"
    assert rb <= 1.0, f"db: worst ratio {rb:.3f}"
