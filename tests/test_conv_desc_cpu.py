"""The convolution descriptors the product builds (ops/_engine.py: the tap tables and the `_*_desc` builders), executed without a GPU by
tests/conv_desc_ref.py and held against torch in f64.  Inputs are integers in [-3, 3], so every sum is exact and the comparisons are
equalities; every case must also write each destination pixel exactly once.  The weight-gradient descriptor is held, field by field,
against the one tests/wgrad_ref.py restates for its model of the dispatch."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_desc_ref as I
import wgrad_ref as R
import xmc_gan_amd.lib as L
from xmc_gan_amd.ops import _engine as E
from xmc_gan_amd.ops._config import chan_pad, pad_to

N, CIN, COUT = 2, 3, 2
# (k, s, p, H, W): maps of 3 to 6 pixels, even where the stride is 2
GEOMS = [(3, 1, 1, 5, 6), (4, 2, 1, 6, 4), (1, 1, 0, 3, 4), (2, 2, 0, 4, 6), (3, 1, 0, 5, 4)]
GEOM_IDS = [f"k{k}s{s}p{p}-{H}x{W}" for k, s, p, H, W in GEOMS]


def ints(*shape, seed):
    return torch.randint(-3, 4, shape, generator=torch.Generator().manual_seed(seed)).double()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def fwd_slices(w, rows):
    """[Co, Ci, kh, kw] -> [kh*kw, rows, Ci] in the weight's row-major tap order, zero rows past Co (the stored channels of y)"""
    co, ci, kh, kw = w.shape
    out = np.zeros((kh * kw, rows, ci))
    out[:, :co] = w.permute(2, 3, 0, 1).reshape(kh * kw, co, ci).numpy()
    return out


def run_once(d, src, slices):
    """the interpreter's result; every destination pixel written exactly once is a condition of every case"""
    dst, writes = I.run(d, src, slices)
    assert (writes == 1).all(), writes
    return dst


def assert_fwd(dst, y):
    """dst [N, OH, OW, pad8(Co)] against y [N, Co, OH, OW]: equal, and zero in the padding channels"""
    assert dst.shape[:3] == nhwc(y).shape[:3]
    assert np.array_equal(dst[..., :y.shape[1]], nhwc(y)) and not dst[..., y.shape[1]:].any()


# ------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("k,s,p,H,W", GEOMS, ids=GEOM_IDS)
def test_forward_equals_conv2d(k, s, p, H, W):
    x, w = ints(N, CIN, H, W, seed=1), ints(COUT, CIN, k, k, seed=2)
    d = E._fwd_desc(E.ConvGeom(CIN, COUT, k, s, p), N, H, W, CIN, L.F32, L.F32)
    assert_fwd(run_once(d, nhwc(x), fwd_slices(w, d.CD)), F.conv2d(x, w, None, s, p))


def test_forward_non_square_kernel():
    x, w = ints(N, CIN, 3, 6, seed=3), ints(COUT, CIN, 1, 7, seed=4)
    d = E._fwd_desc(E.ConvGeom(CIN, COUT, (1, 7), 1, (0, 3)), N, 3, 6, CIN, L.F32, L.F32)
    assert (d.ntaps, d.DH, d.DW) == (7, 3, 6)
    assert_fwd(run_once(d, nhwc(x), fwd_slices(w, d.CD)), F.conv2d(x, w, None, 1, (0, 3)))


def test_forward_tap_ranges_sum_to_the_5x5_kernel():
    x, w = ints(N, CIN, 5, 6, seed=5), ints(COUT, CIN, 5, 5, seed=6)
    geom = E.ConvGeom(CIN, COUT, 5, 1, 2)
    with pytest.raises(AssertionError):
        E._fwd_desc(geom, N, 5, 6, CIN, L.F32, L.F32)                 # 25 taps do not fit one descriptor
    parts = []
    for rng in ((0, 16), (16, 25)):
        d = E._fwd_desc(geom, N, 5, 6, CIN, L.F32, L.F32, taps=rng)
        assert d.ntaps == rng[1] - rng[0] and list(d.wi[0][:d.ntaps]) == list(range(*rng))
        parts.append(run_once(d, nhwc(x), fwd_slices(w, d.CD)))
    assert_fwd(parts[0] + parts[1], F.conv2d(x, w, None, 1, 2))


def test_forward_through_src_shift_equals_conv_of_the_upsampled_map():
    x, w = ints(N, CIN, 3, 4, seed=7), ints(COUT, CIN, 3, 3, seed=8)
    d = E._fwd_desc(E.ConvGeom(CIN, COUT, 3, 1, 1), N, 3, 4, CIN, L.F32, L.F32, up=True)
    assert (d.src_shift, d.SH, d.SW, d.DH, d.DW) == (1, 3, 4, 6, 8)
    assert_fwd(run_once(d, nhwc(x), fwd_slices(w, d.CD)), F.conv2d(F.interpolate(x, scale_factor=2), w, None, 1, 1))


# ------------------------------------------------------------------------------------------ data gradient
@pytest.mark.parametrize("k,s,p,H,W", GEOMS, ids=GEOM_IDS)                # k % s == 0 in all five
def test_data_gradient_equals_autograd(k, s, p, H, W):
    geom = E.ConvGeom(CIN, COUT, k, s, p)
    OH, OW = geom.out_hw(H, W)
    x, w, dy = ints(N, CIN, H, W, seed=9).requires_grad_(), ints(COUT, CIN, k, k, seed=10), ints(N, COUT, OH, OW, seed=11)
    dx, = torch.autograd.grad(F.conv2d(x, w, None, s, p), x, dy)
    d = E._dgrad_geom_desc(geom, N, OH, OW, COUT, H, W, CIN, L.F32, L.F32)
    assert (d.nclass, d.DA, d.MH, d.MW) == (s * s, s, H // s, W // s)
    slices = w.permute(2, 3, 1, 0).reshape(k * k, CIN, COUT).numpy()            # transposed: [tap][ci][co]
    assert np.array_equal(run_once(d, nhwc(dy), slices), nhwc(dx))


# ------------------------------------------------------------------------------------------ fused upsample
def test_fused_upsample_forward_and_data_gradient():
    H, W = 3, 4
    geom = E.ConvGeom(CIN, COUT, 3, 1, 1)
    x, w, dy = ints(N, CIN, H, W, seed=12).requires_grad_(), ints(COUT, CIN, 3, 3, seed=13), ints(N, COUT, 2 * H, 2 * W, seed=14)
    y = F.conv2d(F.interpolate(x, scale_factor=2), w, None, 1, 1)
    dx, = torch.autograd.grad(y, x, dy)
    pre = I.upconv_slices(w.numpy())                                             # [16, Co, Ci]
    d = E._upconv_fwd_desc(geom, N, H, W, CIN, L.F32, L.F32)
    assert (d.nclass, d.ntaps, d.DA, d.DH, d.DW) == (4, 4, 2, 2 * H, 2 * W)
    padded = np.zeros((16, d.CD, CIN))
    padded[:, :COUT] = pre
    assert_fwd(run_once(d, nhwc(x.detach()), padded), y.detach())
    d = E._upconv_dgrad_desc(geom, N, 2 * H, 2 * W, COUT, CIN, L.F32, L.F32)
    assert (d.nclass, d.ntaps, d.SA, d.DH, d.DW) == (1, 16, 2, H, W)
    assert np.array_equal(run_once(d, nhwc(dy), pre.transpose(0, 2, 1)), nhwc(dx))


# ------------------------------------------------------------------------------------------ weight gradient
RUNS = R.all_runs()


@pytest.mark.parametrize("run", RUNS, ids=[f"{t}-{R.case_id(e.case)}-{mode}" for t, e, mode in RUNS])
def test_weight_gradient_descriptor_is_the_one_the_dispatch_model_reads(run):
    _, e, mode = run
    c, m = e.case, R.desc(e.case, mode)
    geom = E.ConvGeom(c.cin, c.cout, c.k, c.s, c.p, groups=c.groups)
    OH, OW = geom.out_hw(c.H << int(c.up), c.W << int(c.up))
    d = E._wgrad_desc(geom, c.N, c.H, c.W, chan_pad(c.cin, R.DTYPE[mode]), OH, OW, pad_to(c.cout, 8), L.F32 if mode == "fp32" else L.BF16, c.up)
    for f in ("N", "SH", "SW", "CS", "CD", "CDw", "MH", "MW", "SA", "src_shift", "ntaps", "groups"):
        assert getattr(d, f) == m[f], (f, getattr(d, f), m[f])
    assert (d.dtype == L.F32) == m.f32 and d.N * d.MH * d.MW == m.P
    assert list(d.dh[0][:d.ntaps]) == m.dh and list(d.dw[0][:d.ntaps]) == m.dw and list(d.wi[0][:d.ntaps]) == list(range(d.ntaps))
    assert (d.nclass, d.DA, d.DH, d.DW, d.out_dtype) == (1, 1, OH, OW, L.F32)


def test_the_table_has_its_55_cases():
    assert len({e.case for _, es, _ in R.TABLES for e in es}) == 55


# ------------------------------------------------------------------------------------------ struct hygiene, refusals
def _built():
    g3, g4 = E.ConvGeom(CIN, COUT, 3, 1, 1), E.ConvGeom(CIN, COUT, 4, 2, 1)
    g5 = E.ConvGeom(CIN, COUT, 5, 1, 2, groups=1)
    return {
        "fwd": (E._fwd_desc(g3, N, 5, 6, 8, L.BF16, L.F32, up=True), E._fwd_classes(g3)),
        "fwd-range": (E._fwd_desc(g5, N, 5, 6, 8, L.BF16, L.BF16, taps=(16, 25)), E._fwd_classes(g5, (16, 25))),
        "dgrad-s2": (E._dgrad_geom_desc(g4, N, 3, 2, 8, 6, 4, 8, L.BF16, L.BF16), E._dgrad_classes(g4)),
        "dgrad-s1": (E._dgrad_geom_desc(g3, N, 5, 6, 8, 5, 6, 8, L.F32, L.F32), E._dgrad_classes(g3)),
        "wgrad": (E._wgrad_desc(g4, N, 6, 4, 8, 3, 2, 8, L.BF16), E._fwd_classes(g4)),
        "upconv-fwd": (E._upconv_fwd_desc(g3, N, 3, 4, 8, L.BF16, L.BF16), E._upconv_fwd_classes()),
        "upconv-dgrad": (E._upconv_dgrad_desc(g3, N, 6, 8, 8, 8, L.BF16, L.BF16), E._upconv_dgrad_classes()),
    }


BUILT = _built()


@pytest.mark.parametrize("name", sorted(BUILT))
def test_builders_fill_the_tap_fields_and_leave_every_pointer_null(name):
    d, classes = BUILT[name]
    pointers = [f for f, t in L.ConvDesc._fields_ if t is ctypes.c_void_p]
    assert {"src", "wpk", "dst", "splitk_ws", "wpk_lo"} <= set(pointers)
    assert all(getattr(d, f) is None for f in pointers), [f for f in pointers if getattr(d, f) is not None]
    assert d.splitk_ws_bytes == 0
    assert d.nclass == len(classes) <= L.MAX_CLASSES and 1 <= d.ntaps <= L.MAX_TAPS
    for z in range(L.MAX_CLASSES):
        dph, dpw, taps = classes[z] if z < d.nclass else (0, 0, [])
        assert (d.dph[z], d.dpw[z]) == (dph, dpw)
        assert z >= d.nclass or len(taps) == d.ntaps
        want = list(taps) + [(0, 0, 0)] * (L.MAX_TAPS - len(taps))              # slots past ntaps, classes past nclass: zero
        assert [(d.dh[z][t], d.dw[z][t], d.wi[z][t]) for t in range(L.MAX_TAPS)] == want


def test_tap_tables_are_plain_integers():
    for _, classes in BUILT.values():
        for dph, dpw, taps in classes:
            assert all(type(v) is int for v in (dph, dpw) + tuple(v for tap in taps for v in tap))


@pytest.mark.parametrize("k,s,p", [(3, 2, 1), ((1, 7), 1, (0, 3)), (5, 1, 2)], ids=["k-not-multiple-of-s", "non-square", "more-than-MAX_TAPS"])
def test_data_gradient_table_refuses(k, s, p):
    with pytest.raises(AssertionError, match="data gradient: square kernel, k % s == 0"):
        E._dgrad_classes(E.ConvGeom(CIN, COUT, k, s, p))
