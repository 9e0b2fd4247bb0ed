"""tests/wgrad_ref.py checked without a GPU: the f64 reference against f64 autograd, every case of the tables against the kernel and
the regime it names on the model of the dispatch, the conditions under which classes I and II are exact, and that every
instantiation the dispatch can reach is the prediction of a case."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_ref as R

RUNS = R.all_runs()
RUN_IDS = [f"{t}-{R.case_id(e.case)}-{mode}" for t, e, mode in RUNS]


# ------------------------------------------------------------------------------------------ reference against autograd
@pytest.mark.parametrize("c", [R.C(6, 4, 3, 1, 1, 2, 5, 7), R.C(6, 4, 4, 2, 1, 2, 6, 10), R.C(5, 3, 1, 1, 0, 2, 4, 3),
                               R.C(6, 4, 3, 1, 1, 2, 3, 5, up=True), R.C(32, 32, 3, 1, 1, 2, 4, 5, groups=16),
                               R.C(3, 2, 4, 2, 1, 1, 7, 9)], ids=R.case_id)
def test_reference_equals_f64_autograd(c):
    g = R.gen_for("autograd", tuple(c))
    xs, ys = R.shapes(c)
    x, dy = torch.randn(xs, generator=g, dtype=torch.float64), torch.randn(ys, generator=g, dtype=torch.float64)
    w = torch.zeros(c.cout, c.cin // c.groups, c.k, c.k, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(c.cout, dtype=torch.float64, requires_grad=True)
    src = F.interpolate(x, scale_factor=2) if c.up else x
    y = F.conv2d(src, w, b, c.s, c.p, groups=c.groups)
    assert y.shape == dy.shape
    (y * dy).sum().backward()
    dW, db = R.wgrad_ref(x, dy, c.k, c.s, c.p, c.up, c.groups)
    assert dW.shape == w.grad.shape
    for got, ref in ((dW, w.grad), (db, b.grad)):
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_dt_codes_come_from_the_header():
    assert {R.XMC_BF16, R.XMC_F32} == {0, 1} and R.XMC_BF16 != R.XMC_F32
    assert R.predict_kernel(R.SPLITK[0].case, "bf16").startswith("wgrad_kernel<%d, " % R.XMC_BF16)
    assert R.predict_kernel(R.SPLITK[0].case, "fp32").startswith("wgrad_kernel<%d, " % R.XMC_F32)


# ------------------------------------------------------------------------------------------ the tables on the model
@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
def test_case_reaches_its_kernel_and_regime(run):
    _, e, mode = run
    m = R.predict(e.case, mode)
    assert m.kernel == R.expected_kernel(e, mode), (m.kernel, e.why)
    assert e.regime(m), (e.why, {k: v for k, v in m.items() if k != "walks"})


@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
def test_class_one_is_exact(run):
    """9 P < 2^24: every partial sum of products of integers in [-3, 3], in any order, is an integer f32 holds"""
    _, e, mode = run
    d = R.desc(e.case, mode)
    assert 9 * d.N * d.MH * d.MW < 2 ** 24
    x, dy = R.ints(e.case)
    assert float(x.abs().max()) <= 3 and float(dy.abs().max()) <= 3
    for t in (x, dy):
        assert torch.equal(R.rt(t, mode), t)


@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
def test_class_two_probes(run):
    _, e, mode = run
    c = e.case
    m = R.predict(c, mode)
    pr = R.probes(c, mode)
    assert len(pr) >= 4 or m.d.MH * m.d.MW == 1
    for name, (n, a, b) in pr.items():
        assert 0 <= n < c.N and 0 <= a < m.d.MH and 0 <= b < m.d.MW, name
    assert (c.N - 1, m.d.MH - 1, m.d.MW - 1) in pr.values()          # pixel P - 1
    names = set(pr)
    if m.family in ("tile", "tile_rr", "up"):
        assert (m.tiles_y > 1) == ("above a tile seam" in names) and (m.tiles_x > 1) == ("left of a tile seam" in names)
        if m.tiles_y > 1:
            assert pr["above a tile seam"][1] // m.TH + 1 == pr["below a tile seam"][1] // m.TH
        if m.tiles_x > 1:
            assert pr["left of a tile seam"][2] // m.TW + 1 == pr["right of a tile seam"][2] // m.TW
    if m.family in ("splitk", "row") and m.nsplit > 1:
        MHW = m.d.MH * m.d.MW
        lin = lambda q: q[0] * MHW + q[1] * m.d.MW + q[2]
        assert m.ppb - 1 in [lin(q) for q in pr.values()] and m.ppb in [lin(q) for q in pr.values()]
    if not c.up:
        for name, (n, i, j) in R.x_probes(c, mode).items():
            assert 0 <= n < c.N and 0 <= i < c.H and 0 <= j < c.W, name
            assert R.x_fanout(c, i, j) <= 1, name
    else:
        assert R.x_fanout(c, 1, 1) > 1          # why the cases through the upsample run no x-impulses


def test_row_case_has_a_k_step_across_two_images():
    e = R.ROW[0]
    assert "first pixel of a K step that starts mid-image" in R.probes(e.case, "bf16")
    assert R.probes(e.case, "bf16")["first pixel of the image a K step runs into"] == (1, 0, 0)


def test_class_three_covers_every_family_and_mode():
    seen = {(R.predict(e.case, mode).family, mode) for e, modes in R.CLASS3 for mode in modes}
    assert seen == {("splitk", m) for m in R.MODES} | {(f, m) for f in ("tile", "tile_rr", "row", "up") for m in R.H16}


# ------------------------------------------------------------------------------------------ coverage of the dispatch
def _k(dt, *t):
    return "wgrad_kernel<%d, %d, %d, %d, %d, %d>" % ((dt,) + t)


# every instantiation the dispatch code launches with XMC_DEBUG_DISPATCH unset, as the string xmc_note_kernel records
REACHABLE = (
    # conv_wgrad.hip dispatch<XMC_BF16>
    [_k(R.XMC_BF16, *t) for t in ((32, 64, 1, 4, 32), (32, 32, 2, 2, 32), (128, 128, 2, 2, 64), (128, 64, 4, 1, 64), (128, 32, 4, 1, 64),
                                  (64, 64, 2, 2, 64), (64, 32, 2, 2, 32))] +
    # dispatch<XMC_F32>: KPB = 32 and no 128 x 128 form
    [_k(R.XMC_F32, *t) for t in ((32, 64, 1, 4, 32), (32, 32, 2, 2, 32), (128, 64, 4, 1, 32), (128, 32, 4, 1, 32), (64, 64, 2, 2, 32),
                                 (64, 32, 2, 2, 32))] +
    # conv_wgrad_tile.hip: row-reuse forms, stride-2 forms, 16 x 16 tiles, the 8-wave (2, 4) / (4, 2), WT_CASE, diagonal, 64 x 64
    ["wgrad_tile_rr_kernel<4, 4, 2>", "wgrad_tile_rr_kernel<2, 4, 2>", "wgrad_tile_rr_kernel<4, 2, 4>",
     "wgrad_tile_kernel<4, 2, 512, 2, 16, 4>", "wgrad_tile_kernel<2, 1, 256, 2, 16, 2>",
     "wgrad_tile_kernel<4, 4, 512, 1, 9, 4, false, true>",
     "wgrad_tile_kernel<2, 4, 512, 1, 9, 2>", "wgrad_tile_kernel<4, 2, 512, 1, 9, 4>",
     "wgrad_tile_kernel<1, 2, 256, 1, 9, 1>", "wgrad_tile_kernel<1, 4, 256, 1, 9, 1>", "wgrad_tile_kernel<2, 1, 256, 1, 9, 2>",
     "wgrad_tile_kernel<2, 2, 256, 1, 9, 2>", "wgrad_tile_kernel<4, 1, 256, 1, 9, 2>",
     "wgrad_tile_kernel<4, 4, 512, 1, 9, 4, true>", "wgrad_tile_kernel<4, 4, 512, 1, 9, 4>"] +
    ["wgrad_row_kernel<3, 1, 128>", "wgrad_row_kernel<3, 1, 64>", "wgrad_row_kernel<4, 2, 128>", "wgrad_row_kernel<4, 2, 64>"] +
    ["wgrad_up_kernel<2, true>", "wgrad_up_kernel<2, false>", "wgrad_up_kernel<4, true>", "wgrad_up_kernel<4, false>"])

# instantiated in the source but launched by no descriptor unless a debug switch is set: no case, and why
SHADOWED = {
    "wgrad_tile_kernel<2, 4, 256, 1, 9, 2>": "WT_CASE(2, 4): the 8-wave form in front of it takes every (2, 4) layer (no_wt24_8w)",
    "wgrad_tile_kernel<4, 2, 256, 1, 9, 2>": "WT_CASE(4, 2): the 8-wave form in front of it takes every (4, 2) layer (no_wt24_8w)",
}


def test_every_reachable_instantiation_has_a_case():
    predicted = {R.predict_kernel(e.case, mode) for _, e, mode in RUNS}
    assert len(set(REACHABLE)) == len(REACHABLE)
    assert predicted == set(REACHABLE), (sorted(set(REACHABLE) - predicted), sorted(predicted - set(REACHABLE)))
    assert not predicted & set(SHADOWED)
    # the branch of dispatch<DT> that shares its instantiations with the small-P one has a case of its own, in every mode
    assert {mode for _, e, mode in RUNS if R.predict(e.case, mode).get("branch") == "CDw%32"} == set(R.MODES)
