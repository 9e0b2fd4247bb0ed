"""f64 reference, a model of the dispatch and the case tables for the convolution weight-gradient kernels (csrc/conv_wgrad.hip,
conv_wgrad_tile.hip, conv_wgrad_row.hip, conv_wgrad_up.hip); a helper, not a test: imports torch only and runs without a GPU.

Reference.  `wgrad_ref`: dW[co, ci, kh, kw] = sum_{n,a,b} dy[n, co, a, b] X[n, ci, a s + kh - p, b s + kw - p] in f64, one tap at a
time from shifted slices and einsum; X is zero outside the map and, with `up`, the nearest x2 upsample of x.

Dispatch model.  `predict(case, mode)` restates, as integer arithmetic on the descriptor `_conv_wgrad_raw` fills, the accept conditions
of xmc_conv_wgrad_up_try, wgrad_tile_go, xmc_conv_wgrad_row_try and dispatch<DT>, in the order xmc_conv_wgrad tries them, and
the launch geometry of whichever accepts: the exact string xmc_note_kernel records and KP / nsplit / ppb (split-K and row kernels),
seg / nseg (row kernel), tiles_y / tiles_x / ntiles / grid width and the tiles each workgroup of the persistent grid walks (tile and
up kernels).  The XMC_DEBUG_DISPATCH switches are taken as unset.

Inputs, all exactly representable in the mode's storage format, for which the CORRECT f32 result is exact, so that the comparison is
bitwise whatever the order of the additions:
  class I    x, dy independent uniform integers in [-3, 3]: every partial sum is an integer of magnitude <= 9 P < 2^24;
  class II   one operand dense Gaussian, the other zero except at one pixel: every dW element is zero or ONE product (16-bit
             operands: exact in f32; f32 operands: rounded once, by fma(a, b, 0) as by rounding the exact f64 product);
  class III  both dense Gaussian, against |got - ref| <= P 2^-23 sum|x dy| per element: the any-order summation bound with one f32
             ulp (taken at 2^-23) per addition.  It is there for an accumulator narrower than f32, which class I cannot show.

Case tables.  (cin, cout, k, s, p, N, H, W, up, groups), the kernel the case is there for and its regime as a predicate on the model;
tests/test_wgrad_cpu.py holds every entry to both."""
import collections
import os
import re
import zlib

import torch

MODES = ("fp32", "bf16", "f16")
DTYPE = {"fp32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
MAX_DYN_LDS = 160 * 1024 - 1024                # common.h: XMC_MAX_DYN_LDS
BIAS_REPLICAS = 16

Case = collections.namedtuple("Case", "cin cout k s p N H W up groups")


def C(cin, cout, k, s, p, N, H, W, up=False, groups=1):
    return Case(cin, cout, k, s, p, N, H, W, up, groups)


def case_id(c):
    return f"{c.cin}-{c.cout}-k{c.k}s{c.s}p{c.p}-N{c.N}-{c.H}x{c.W}" + ("-up" if c.up else "") + (f"-g{c.groups}" if c.groups > 1 else "")


def _header_enum(name):
    """the value the header gives an enumerator (XMC_BF16 / XMC_F32: what a kernel name prints for its DT argument)"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "xmc_gan_hip.h")
    with open(path) as f:
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, f.read())
    return int(m.group(1))


XMC_BF16, XMC_F32 = _header_enum("XMC_BF16"), _header_enum("XMC_F32")


# ------------------------------------------------------------------------------------------ reference
def out_hw(c):
    vh, vw = (2 * c.H, 2 * c.W) if c.up else (c.H, c.W)
    return (vh + 2 * c.p - c.k) // c.s + 1, (vw + 2 * c.p - c.k) // c.s + 1


def wgrad_ref(x, dy, k, s, p, up=False, groups=1):
    """x [N, Ci, H, W], dy [N, Co, OH, OW] -> dW [Co, Ci / groups, k, k], db [Co], in f64"""
    x, dy = x.double(), dy.double()
    if up:
        x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    N, Ci, H, W = x.shape
    _, Co, OH, OW = dy.shape
    hi_h, hi_w = (OH - 1) * s + k - 1 - p, (OW - 1) * s + k - 1 - p           # the largest source index a tap addresses
    X = torch.zeros(N, Ci, p + max(hi_h + 1, H), p + max(hi_w + 1, W), dtype=torch.float64)
    X[:, :, p:p + H, p:p + W] = x
    g = groups
    dW = torch.zeros(Co, Ci // g, k, k, dtype=torch.float64)
    dyg = dy.reshape(N, g, Co // g, OH, OW)
    for kh in range(k):
        for kw in range(k):
            xs = X[:, :, kh:kh + (OH - 1) * s + 1:s, kw:kw + (OW - 1) * s + 1:s]      # X[n, ci, a s + kh - p, b s + kw - p]
            dW[:, :, kh, kw] = torch.einsum("ngoab,ngiab->goi", dyg, xs.reshape(N, g, Ci // g, OH, OW)).reshape(Co, Ci // g)
    return dW, dy.sum(dim=(0, 2, 3))


def class3_bound(x, dy, c):
    """P 2^-23 sum|x dy| over each element's own terms"""
    S, Sb = wgrad_ref(x.abs(), dy.abs(), c.k, c.s, c.p, c.up, c.groups)
    P = dy.shape[0] * dy.shape[2] * dy.shape[3]
    return P * 2.0 ** -23 * S, P * 2.0 ** -23 * Sb


# ------------------------------------------------------------------------------------------ inputs
def gen_for(*key):
    """a generator seeded by the case, the same on every machine"""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def rt(t, mode):
    """round to the storage format of `mode`, held in f64"""
    return t.float().to(DTYPE[mode]).double()


def shapes(c):
    OH, OW = out_hw(c)
    return (c.N, c.cin, c.H, c.W), (c.N, c.cout, OH, OW)


def ints(c):
    """class I: the same integers in every mode (all of them are exact in bf16)"""
    g = gen_for("ints", tuple(c))
    xs, ys = shapes(c)
    return torch.randint(-3, 4, xs, generator=g).double(), torch.randint(-3, 4, ys, generator=g).double()


def gauss(c, mode):
    """classes II and III: dense Gaussian operands rounded to the format"""
    g = gen_for("gauss", tuple(c), mode)
    xs, ys = shapes(c)
    return rt(torch.randn(xs, generator=g), mode), rt(torch.randn(ys, generator=g), mode)


def impulse_values(c, mode, which, probe):
    """the channel vector an impulse holds at its pixel: Gaussian with full mantissas"""
    g = gen_for("impulse", tuple(c), mode, which, probe)
    return rt(torch.randn(c.cin if which == "x" else c.cout, generator=g), mode)


# ------------------------------------------------------------------------------------------ dispatch model
def cdiv(a, b):
    return -(-a // b)


def pad_to(n, m):
    return cdiv(n, m) * m


def chan_pad(c, mode):
    """ops.chan_pad: stored channels of an activation"""
    return c if (mode == "fp32" and c % 4 == 0) else pad_to(c, 8)


class Model(dict):
    __getattr__ = dict.__getitem__


def desc(c, mode):
    """the XmcConvDesc fields `_conv_wgrad_raw` fills that the dispatch reads"""
    MH, MW = out_hw(c)
    CD = pad_to(c.cout, 8)
    taps = [(kh - c.p, kw - c.p) for kh in range(c.k) for kw in range(c.k)]
    return Model(f32=mode == "fp32", N=c.N, SH=c.H, SW=c.W, CS=chan_pad(c.cin, mode), CD=CD, CDw=pad_to(CD, 32), MH=MH, MW=MW, SA=c.s,
                 src_shift=1 if c.up else 0, ntaps=c.k * c.k, groups=c.groups, dh=[t[0] for t in taps], dw=[t[1] for t in taps],
                 P=c.N * MH * MW)


def xcd_walk(G, b, ntiles):
    """common.h xmc_xcd_walk: the tiles workgroup b of a persistent grid of G walks"""
    if (G & 7) != 0 or G < 16:
        return list(range(b, ntiles, G))
    T8 = (ntiles + 7) >> 3
    base = (b & 7) * T8
    return list(range(base + (b >> 3), min(base + T8, ntiles), G >> 3))


def _persistent(m, gx):
    """grid width and walk of the tile / up kernels (xmc_ab_grid is the identity without its debug switch)"""
    gx = min(max(gx, 1), m["ntiles"])
    m["grid"] = (gx, m["ny"], m["nz"])
    m["walks"] = [xcd_walk(gx, b, m["ntiles"]) for b in range(gx)]
    return m


def _std33(d):
    return d.ntaps == 9 and all(d.dh[t] == t // 3 - 1 and d.dw[t] == t % 3 - 1 for t in range(9))


def _up_try(d):
    if d.f32 or d.src_shift != 1 or d.SA != 1 or d.ntaps != 9 or d.groups > 1:
        return None
    if d.MH != 2 * d.SH or d.MW != 2 * d.SW:
        return None
    if d.CS % 64 != 0 or not (d.CD == 32 or d.CD % 64 == 0):
        return None
    if not _std33(d):
        return None
    w16 = d.SW % 32 != 0
    if (d.SW % 16 != 0 or d.SH % 8 != 0) if w16 else (d.SH % 4 != 0):
        return None
    TLH, TLW = (8, 16) if w16 else (4, 32)
    nco = 2 if d.CD == 32 else 4
    lds = 4 * 128 * (nco * 32 + 32) + (TLH + 2) * (TLW + 2) * 160
    if lds > MAX_DYN_LDS:
        return None
    m = Model(family="up", kernel="wgrad_up_kernel<%d, %s>" % (nco, "true" if w16 else "false"), TH=2 * TLH, TW=2 * TLW,
              tiles_y=d.SH // TLH, tiles_x=d.SW // TLW, ny=d.CS // 64, nz=cdiv(d.CD, 64))
    m["ntiles"] = d.N * m.tiles_y * m.tiles_x
    return _persistent(m, 256 // (m.ny * m.nz))


def _wt_occ(nco, nci):
    return 4 if (nco, nci) == (2, 1) else 3 if (nco * nci <= 2 or (nco, nci) == (2, 2)) else 2 if nco * nci == 8 else 1


def _tile_try(d, want_bias):
    if d.f32 or d.src_shift not in (0, 1):
        return None
    s2 = d.SA == 2
    if d.SA != 1 and not (s2 and d.ntaps == 16 and d.src_shift == 0 and d.CS <= 32):
        return None
    wide = d.CD > 64 or d.CS > 64
    if wide and (s2 or (d.CD > 64 and d.CD % 64) or (d.CS > 64 and d.CS % 64)):
        return None
    if d.ntaps > (16 if s2 else 9) or d.ntaps < 1:
        return None
    t16 = d.MW % 32 != 0 and d.MW % 16 == 0 and d.MH % 16 == 0 and not s2 and d.ntaps >= 4
    TH, TW = (16, 16) if t16 else (8, 32)
    if d.MW % TW != 0 or d.MH % TH != 0:
        return None
    if d.CD % 8 != 0 or d.CS % 8 != 0:
        return None
    PH = d.SA * (TH - 1) + (max(d.dh) - min(d.dh) + 1)
    PW = d.SA * (TW - 1) + (max(d.dw) - min(d.dw) + 1)
    if (PH > 18 or PW > 66 or (PW & 1)) if s2 else (PH > 18 or PW > 18) if t16 else (PH > 10 or PW > 34):
        return None
    nco = 1 if d.CD <= 16 else 2 if d.CD <= 32 else 4
    nci = 1 if d.CS <= 16 else 2 if d.CS <= 32 else 4
    m = Model(TH=TH, TW=TW, PH=PH, PW=PW, tiles_y=d.MH // TH, tiles_x=d.MW // TW, ny=cdiv(d.CS, 64), nz=cdiv(d.CD, 64))
    m["ntiles"] = d.N * m.tiles_y * m.tiles_x
    lds = lambda ph, pw: 256 * (nco * 32 + 32) + ph * pw * (nci * 32 + 32)

    def wt(nt, sa, kt, cbw, diag=False, t16_=False):
        if lds(PH, PW) > MAX_DYN_LDS:
            return None
        per_cu = min(160 * 1024 // lds(PH, PW), 3 if _wt_occ(nco, nci) >= 3 else 2)
        if nt == 512:
            per_cu = 1
        if diag:
            m["nz"] = 1
        m["family"] = "tile"
        m["kernel"] = "wgrad_tile_kernel<%d, %d, %d, %d, %d, %d%s>" % (nco, nci, nt, sa, kt, cbw,
                                                                        ", false, true" if t16_ else ", true" if diag else "")
        return _persistent(m, 256 * per_cu // (m.ny * m.nz))

    if s2:
        if (nco, nci) == (4, 2):
            return wt(512, 2, 16, 4)
        if (nco, nci) == (2, 1):
            return wt(256, 2, 16, 2)
        return None
    if t16:
        return wt(512, 1, 9, 4, t16_=True) if (nco, nci) == (4, 4) else None
    if _std33(d) and PH == 10 and PW == 34 and d.groups <= 1 and (nco, nci) in ((4, 4), (2, 4), (4, 2)):
        if lds(10, 34) > MAX_DYN_LDS:
            return None
        m["family"] = "tile_rr"
        m["kernel"] = "wgrad_tile_rr_kernel<%d, %d, %d>" % (nco, nci, 4 if (nco, nci) == (4, 2) else 2)
        return _persistent(m, 256 // (m.ny * m.nz))
    if (nco, nci) == (2, 4):
        return wt(512, 1, 9, 2)
    if (nco, nci) == (4, 2):
        return wt(512, 1, 9, 4)
    if (nco, nci) in ((1, 2), (1, 4), (2, 1), (2, 2), (4, 1)):
        return wt(256, 1, 9, 2 if nco >= 2 else 1)
    if (nco, nci) == (4, 4):
        if (d.groups > 1 and d.CD == d.CS and d.CD % 64 == 0 and d.CD % d.groups == 0 and 16 % (d.CD // d.groups) == 0
                and not want_bias):
            return wt(512, 1, 9, 4, diag=True)
        return wt(512, 1, 9, 4)
    return None


def _row_try(d):
    if d.f32 or (d.src_shift != 0 and d.SA != 1):
        return None
    if (d.CS % 128 != 0 and d.CS != 64) or d.CD % 128 != 0 or d.CDw != d.CD:
        return None
    if d.ntaps == 9 and d.SA == 1:
        kw, sa = 3, 1
    elif d.ntaps == 16 and d.SA == 2:
        kw, sa = 4, 2
    else:
        return None
    pad = -d.dh[0]
    if pad < 0 or pad > 2 or any(d.dh[t] != t // kw - pad or d.dw[t] != t % kw - pad for t in range(d.ntaps)):
        return None
    W = d.MW
    if W < 4 or (W & (W - 1)) != 0:
        return None
    if d.P % 64 != 0 or d.P < 256:
        return None
    seg = min(W, 64)
    nseg = 64 // seg
    xseg = sa * (seg - 1) + kw
    bci = 64 if d.CS == 64 else 128
    if 2 * (64 * 144 + nseg * xseg * (bci + 16 if sa == 1 else bci + 8)) * 2 > MAX_DYN_LDS:
        return None
    tiles = (d.CDw // 128) * (d.CS // bci) * kw
    nsplit = max(256 // tiles, 1)
    nsplit = min(nsplit, max(d.P // 256, 1))
    ppb = pad_to(cdiv(d.P, nsplit), 64)
    nsplit = cdiv(d.P, ppb)
    return Model(family="row", kernel="wgrad_row_kernel<%d, %d, %d>" % (kw, sa, bci), KP=64, nsplit=nsplit, ppb=ppb, seg=seg, nseg=nseg,
                 grid=(nsplit, (d.CDw // 128) * (d.CS // bci), kw))


def _splitk(d):
    DT = XMC_F32 if d.f32 else XMC_BF16
    KPB = 32 if d.f32 else 64
    wide_ci = d.CS > 32
    small = (32, 64, 1, 4, 32) if wide_ci else (32, 32, 2, 2, 32)
    if d.P <= 1024:
        t, branch = small, "small-P"
    elif d.CDw % 128 == 0:
        t = (128, 128, 2, 2, KPB) if (d.CS % 128 == 0 and not d.f32) else (128, 64, 4, 1, KPB) if wide_ci else (128, 32, 4, 1, KPB)
        branch = "CDw%128"
    elif d.CDw % 64 == 0:
        t, branch = ((64, 64, 2, 2, KPB) if wide_ci else (64, 32, 2, 2, 32)), "CDw%64"
    else:
        t, branch = small, "CDw%32"
    BCO, BCI, _, _, KP = t
    nci = cdiv(d.CS, BCI)
    tiles = (d.CDw // BCO) * nci * d.ntaps
    nsplit = max(min(cdiv(1024, tiles), cdiv(d.P, 4 * KP)), 1)
    ppb = pad_to(cdiv(d.P, nsplit), KP)
    nsplit = cdiv(d.P, ppb)
    return Model(family="splitk", kernel="wgrad_kernel<%d, %d, %d, %d, %d, %d>" % ((DT,) + t), branch=branch, BCO=BCO, BCI=BCI, KP=KP,
                 nsplit=nsplit, ppb=ppb, nco_blocks=d.CDw // BCO, nci_blocks=nci, grid=(nsplit, (d.CDw // BCO) * nci, d.ntaps))


def want_bias(c):
    """`_wgrad_unpack` has no bias path for a grouped layer"""
    return c.groups == 1


def predict(c, mode):
    """the kernel xmc_conv_wgrad launches for the case, and its geometry; m.declined: the families tried before it"""
    d = desc(c, mode)
    declined = []
    for name, m in (("up", lambda: _up_try(d)), ("tile", lambda: _tile_try(d, want_bias(c))), ("row", lambda: _row_try(d)),
                    ("splitk", lambda: _splitk(d))):
        r = m()
        if r is not None:
            r["declined"] = tuple(declined)
            r["d"] = d
            return r
        declined.append(name)
    raise AssertionError("unreachable")


def predict_kernel(c, mode):
    return predict(c, mode).kernel


# ------------------------------------------------------------------------------------------ class II probe positions
def probes(c, mode):
    """{name: (n, a, b)}: output pixels the model singles out for the case (dy-impulses sit there; x-impulses at the source pixel
    below, `x_probes`)"""
    m = predict(c, mode)
    d = m.d
    MH, MW, MHW, P = d.MH, d.MW, d.MH * d.MW, d.P
    out = collections.OrderedDict()

    def lin(name, q):
        if 0 <= q < P:
            out.setdefault(name, (q // MHW, (q % MHW) // MW, q % MW))

    for n, tag in ((0, "first"), (c.N - 1, "last")):
        for a, b, cn in ((0, 0, "top-left"), (0, MW - 1, "top-right"), (MH - 1, 0, "bottom-left"), (MH - 1, MW - 1, "bottom-right")):
            out[f"{tag} image {cn}"] = (n, a, b)
    if m.family in ("tile", "tile_rr", "up"):
        if m.tiles_y > 1:
            out["above a tile seam"], out["below a tile seam"] = (0, m.TH - 1, min(5, MW - 1)), (0, m.TH, min(5, MW - 1))
        if m.tiles_x > 1:
            out["left of a tile seam"], out["right of a tile seam"] = (c.N - 1, min(3, MH - 1), m.TW - 1), (c.N - 1, min(3, MH - 1), m.TW)
    if m.family in ("splitk", "row") and m.nsplit > 1:
        lin("last pixel of split 0", m.ppb - 1)
        lin("first pixel of split 1", m.ppb)
    if m.family == "row":
        starts = [q for q in range(0, P, 64) if q % MHW != 0]
        if starts:
            lin("first pixel of a K step that starts mid-image", starts[0])
        cross = [q for q in range(0, P, 64) if q // MHW != (q + 63) // MHW]
        if cross:
            lin("first pixel of the image a K step runs into", (cross[0] // MHW + 1) * MHW)
    lin("pixel P - 1", P - 1)
    seen, uniq = set(), collections.OrderedDict()
    for k, v in out.items():
        if v not in seen:
            seen.add(v)
            uniq[k] = v
    return uniq


def x_probes(c, mode):
    """{name: (n, i, j)} source pixels for the x-impulses: below every output probe, and the source map's own corners"""
    out = collections.OrderedDict()
    for k, (n, a, b) in probes(c, mode).items():
        out[k] = (n, min(a * c.s, c.H - 1), min(b * c.s, c.W - 1))
    for n, tag in ((0, "first"), (c.N - 1, "last")):
        out[f"{tag} image source bottom-right"] = (n, c.H - 1, c.W - 1)
    seen, uniq = set(), collections.OrderedDict()
    for k, v in out.items():
        if v not in seen:
            seen.add(v)
            uniq[k] = v
    return uniq


def x_fanout(c, i, j):
    """the largest number of output pixels one tap pairs source pixel (i, j) with"""
    MH, MW = out_hw(c)
    sh = 1 if c.up else 0
    worst = 0
    for kh in range(c.k):
        for kw in range(c.k):
            na = sum(1 for a in range(MH) if 0 <= a * c.s + kh - c.p < (c.H << sh) and (a * c.s + kh - c.p) >> sh == i)
            nb = sum(1 for b in range(MW) if 0 <= b * c.s + kw - c.p < (c.W << sh) and (b * c.s + kw - c.p) >> sh == j)
            worst = max(worst, na * nb)
    return worst


# ------------------------------------------------------------------------------------------ case tables
Entry = collections.namedtuple("Entry", "case kernel kernel32 regime why")


def _k(t, dt=None):
    return "wgrad_kernel<%d, %d, %d, %d, %d, %d>" % ((XMC_BF16 if dt is None else dt,) + t)


def _tile(nco, nci, nt, sa, kt, cbw, tail=""):
    return "wgrad_tile_kernel<%d, %d, %d, %d, %d, %d%s>" % (nco, nci, nt, sa, kt, cbw, tail)


def _rr(*a):
    return "wgrad_tile_rr_kernel<%d, %d, %d>" % a


def _row(*a):
    return "wgrad_row_kernel<%d, %d, %d>" % a


def _declines(m, *fams):
    return all(f in m.declined for f in fams)


def _second_tile_for_some(m):
    n = {len(w) for w in m.walks}
    return m.ntiles > m.grid[0] and min(n) == 1 and max(n) == 2 and sorted(t for w in m.walks for t in w) == list(range(m.ntiles))


def SK(case, t16, t32, regime, why):
    return Entry(case, _k(t16), _k(t32, XMC_F32), regime, why)


# split-K kernel (conv_wgrad.hip): 16-bit modes and fp32 (KPB = 32; nothing else takes fp32)
SPLITK = [
    SK(C(8, 8, 3, 1, 1, 3, 7, 5), (32, 32, 2, 2, 32), (32, 32, 2, 2, 32),
       lambda m: m.branch == "small-P" and m.d.P == 105 and m.d.P % 32 != 0 and m.d.CD == 8 and m.d.CDw == 32,
       "small-P, P = 105 not a multiple of the K step, CD 8 < CDw 32"),
    SK(C(40, 24, 3, 1, 1, 2, 9, 11), (32, 64, 1, 4, 32), (32, 64, 1, 4, 32),
       lambda m: m.branch == "small-P" and m.d.CS == 40 and m.d.CS % m.BCI != 0 and m.d.CD == 24,
       "small-P, CS 40 ragged in a 64 block, CD 24"),
    SK(C(64, 64, 3, 1, 1, 16, 8, 8), (32, 64, 1, 4, 32), (32, 64, 1, 4, 32),
       lambda m: m.branch == "small-P" and m.d.P == 1024, "P = 1024, the small-P boundary itself"),
    SK(C(64, 64, 3, 1, 1, 17, 8, 8), (64, 64, 2, 2, 64), (64, 64, 2, 2, 32),
       lambda m: m.branch == "CDw%64" and m.d.P == 1088 and m.nsplit > 1 and m.d.P % m.ppb != 0, "P = 1088, one image past the boundary"),
    SK(C(72, 96, 3, 1, 1, 5, 15, 15), (32, 64, 1, 4, 32), (32, 64, 1, 4, 32),
       lambda m: m.branch == "CDw%32" and m.d.P > 1024 and m.nco_blocks == 3 and m.nci_blocks == 2 and m.d.CS - m.BCI == 8 and m.d.P % 32 == 5,
       "the CDw % 32 branch at P > 1024: 3 co blocks x 2 ci blocks, the second 8 wide, P % 32 = 5"),
    SK(C(16, 64, 4, 2, 1, 3, 42, 42), (64, 32, 2, 2, 32), (64, 32, 2, 2, 32),
       lambda m: m.branch == "CDw%64" and m.d.SA == 2 and (m.d.MH, m.d.MW) == (21, 21) and (m.d.f32 or _declines(m, "tile")) and m.d.P % m.KP != 0,
       "stride 2 onto 21x21; the stride-2 tile kernel declines on MW % 32"),
    SK(C(64, 192, 1, 1, 0, 2, 23, 25), (64, 64, 2, 2, 64), (64, 64, 2, 2, 32),
       lambda m: m.d.ntaps == 1 and m.d.P % 64 != 0 and m.nco_blocks == 3 and m.d.P > 1024, "1x1, P % 64 != 0, three co blocks"),
    SK(C(128, 128, 3, 1, 1, 5, 20, 12), (128, 128, 2, 2, 64), (128, 64, 4, 1, 32),
       lambda m: m.d.P == 1200 and m.nsplit > 1 and m.d.P % m.ppb != 0 and (m.d.f32 or _declines(m, "tile", "row")),
       "last split partial (P = 1200); fp32 has no 128x128 form"),
    SK(C(64, 128, 3, 1, 1, 5, 20, 12), (128, 64, 4, 1, 64), (128, 64, 4, 1, 32),
       lambda m: m.branch == "CDw%128" and (m.d.f32 or _declines(m, "tile", "row")), "row kernel declines: W = 12 is not a power of two"),
    SK(C(32, 128, 3, 1, 1, 5, 20, 12), (128, 32, 4, 1, 64), (128, 32, 4, 1, 32),
       lambda m: m.branch == "CDw%128" and m.d.CS == 32, "the 32-wide ci block under 128 co"),
    SK(C(64, 96, 3, 1, 1, 2, 16, 32), (32, 64, 1, 4, 32), (32, 64, 1, 4, 32),
       lambda m: m.d.MH % 8 == 0 and m.d.MW % 32 == 0 and m.d.CD == 96 and (m.d.f32 or _declines(m, "tile")),
       "CD 96 > 64 and not a multiple of 64: the tile kernel declines on a tile-shaped map"),
    SK(C(128, 128, 3, 1, 1, 3, 5, 8), (32, 64, 1, 4, 32), (32, 64, 1, 4, 32),
       lambda m: m.d.P % 64 != 0 and m.d.MW == 8 and (m.d.f32 or _declines(m, "row")), "row kernel declines on P % 64"),
    SK(C(128, 128, 3, 1, 1, 1, 12, 16), (32, 64, 1, 4, 32), (32, 64, 1, 4, 32),
       lambda m: m.d.P % 64 == 0 and m.d.P < 256 and (m.d.f32 or _declines(m, "tile", "row")), "row kernel declines on P < 256"),
]

_G = 16
# all-taps tile kernels (conv_wgrad_tile.hip): bf16 and f16
TILE = [
    Entry(C(64, 64, 3, 1, 1, 2, 8, 64), _rr(4, 4, 2), None, lambda m: (m.tiles_y, m.tiles_x) == (1, 2), "one tile row, two tile columns"),
    Entry(C(64, 64, 3, 1, 1, 1, 24, 32), _rr(4, 4, 2), None, lambda m: (m.tiles_y, m.tiles_x) == (3, 1), "top, inner and bottom tile row"),
    Entry(C(64, 64, 3, 1, 1, 33, 64, 32), _rr(4, 4, 2), None, _second_tile_for_some,
          "ntiles > grid width: some workgroups of the persistent grid take a second tile, others do not"),
    Entry(C(64, 24, 3, 1, 1, 2, 16, 32), _rr(2, 4, 2), None, lambda m: m.d.CD == 24 and m.tiles_y == 2, "CD 24 inside a 32 block"),
    Entry(C(32, 64, 3, 1, 1, 2, 16, 32), _rr(4, 2, 4), None, lambda m: m.tiles_y == 2, "four Cout groups x two group slices"),
    Entry(C(128, 128, 3, 1, 1, 2, 16, 32), _rr(4, 4, 2), None, lambda m: (m.ny, m.nz) == (2, 2), "2 x 2 channel blocks over grid.y / grid.z"),
    Entry(C(192, 64, 3, 1, 1, 1, 8, 32), _rr(4, 4, 2), None, lambda m: (m.ny, m.nz) == (3, 1) and m.ntiles == m.d.N,
          "three ci blocks, one tile per image"),
    Entry(C(3, 32, 3, 1, 1, 2, 8, 32), _tile(2, 1, 256, 1, 9, 2), None, lambda m: m.d.CS == 8, "CS 3 -> 8"),
    Entry(C(3, 64, 3, 1, 1, 2, 8, 32), _tile(4, 1, 256, 1, 9, 2), None, lambda m: m.d.CS == 8, "CS 3 -> 8 under 64 co"),
    Entry(C(32, 3, 3, 1, 1, 2, 8, 32), _tile(1, 2, 256, 1, 9, 1), None, lambda m: m.d.CD == 8 and m.d.CDw == 32, "CD 3 -> 8, CDw 32"),
    Entry(C(64, 3, 3, 1, 1, 2, 8, 32), _tile(1, 4, 256, 1, 9, 1), None, lambda m: m.d.CD == 8, "CD 3 -> 8 over 64 ci"),
    Entry(C(32, 32, 3, 1, 1, 2, 16, 32), _tile(2, 2, 256, 1, 9, 2), None, lambda m: m.tiles_y == 2, "the (2, 2) form"),
    Entry(C(8, 8, 3, 1, 1, 2, 8, 32), _k((32, 32, 2, 2, 32)), None, lambda m: _declines(m, "tile", "row"), "(1, 1) has no tile form"),
    Entry(C(64, 32, 1, 1, 0, 2, 8, 32), _tile(2, 4, 512, 1, 9, 2), None, lambda m: (m.PH, m.PW) == (8, 32), "one tap: PH 8, PW 32"),
    Entry(C(32, 64, 1, 1, 0, 2, 8, 32), _tile(4, 2, 512, 1, 9, 4), None, lambda m: (m.PH, m.PW) == (8, 32), "one tap, 8 waves"),
    Entry(C(64, 64, 1, 1, 0, 2, 8, 32), _tile(4, 4, 512, 1, 9, 4), None, lambda m: (m.PH, m.PW) == (8, 32), "one tap, 64 x 64"),
    Entry(C(64, 64, 3, 1, 1, 2, 16, 16), _tile(4, 4, 512, 1, 9, 4, ", false, true"), None, lambda m: (m.TH, m.TW) == (16, 16), "16 x 16 tiles"),
    Entry(C(128, 64, 3, 1, 1, 1, 32, 16), _tile(4, 4, 512, 1, 9, 4, ", false, true"), None,
          lambda m: m.d.MH != m.d.MW and (m.tiles_y, m.tiles_x) == (2, 1) and m.ny == 2, "16 x 16 tiles, wide, MH != MW, two tile rows"),
    Entry(C(64, 64, 3, 1, 1, 2, 16, 48), _tile(4, 4, 512, 1, 9, 4, ", false, true"), None, lambda m: m.d.MW == 48 and m.tiles_x == 3,
          "MW = 48: three tile columns on a width that is not a power of two"),
    Entry(C(32, 64, 3, 1, 1, 2, 16, 16), _k((32, 32, 2, 2, 32)), None, lambda m: _declines(m, "tile", "row"), "16 x 16 tiles need nco = nci = 4"),
    Entry(C(32, 64, 4, 2, 1, 2, 16, 64), _tile(4, 2, 512, 2, 16, 4), None, lambda m: (m.d.MH, m.d.MW) == (8, 32) and (m.PH, m.PW) == (18, 66),
          "stride 2 onto 8x32"),
    Entry(C(16, 32, 4, 2, 1, 2, 32, 64), _tile(2, 1, 256, 2, 16, 2), None, lambda m: (m.d.MH, m.d.MW) == (16, 32) and m.tiles_y == 2,
          "stride 2 onto 16x32, two tile rows"),
    Entry(C(32, 32, 4, 2, 1, 2, 16, 64), _k((32, 32, 2, 2, 32)), None, lambda m: _declines(m, "tile", "row") and (m.d.MH, m.d.MW) == (8, 32),
          "no (2, 2) stride-2 form"),
    Entry(C(128, 128, 3, 1, 1, 2, 8, 32, groups=_G), _tile(4, 4, 512, 1, 9, 4, ", true"), None, lambda m: m.grid[1:] == (2, 1),
          "diagonal blocks only; db not requested (the form requires dbias == NULL)"),
    Entry(C(128, 128, 3, 1, 1, 2, 6, 10, groups=_G), _k((32, 64, 1, 4, 32)), None, lambda m: _declines(m, "tile", "row"),
          "grouped layer on the dense kernel plus xmc_unpack_wgrad with groups"),
]

# one kernel row of taps per workgroup (conv_wgrad_row.hip): bf16 and f16
ROW = [
    Entry(C(128, 128, 3, 1, 1, 4, 12, 8), _row(3, 1, 128), None,
          lambda m: (m.seg, m.nseg) == (8, 8) and any(q // 96 != (q + 63) // 96 for q in range(0, m.d.P, 64)),
          "seg 8; K steps that start in one image and end in the next (H = 12, W = 8)"),
    Entry(C(128, 128, 3, 1, 1, 2, 12, 32), _row(3, 1, 128), None, lambda m: m.seg == 32 and m.d.MH % 8 != 0 and m.nsplit > 1 and m.d.MH != m.d.MW,
          "tile kernel declines on MH % 8; seg 32; split-K seams"),
    Entry(C(128, 256, 3, 1, 1, 1, 6, 64), _row(3, 1, 128), None, lambda m: (m.seg, m.nseg) == (64, 1) and m.grid[1] == 2,
          "seg 64 = one image row; two co blocks"),
    Entry(C(128, 128, 3, 1, 1, 1, 4, 128), _row(3, 1, 128), None, lambda m: m.d.MW > m.KP and m.seg == 64, "rows longer than a K step"),
    Entry(C(128, 128, 3, 1, 1, 2, 8, 16), _row(3, 1, 128), None, lambda m: m.d.P == 256 and m.seg == 16,
          "P = 256, the smallest it takes; 16 x 16 tiles decline on MH % 16"),
    Entry(C(64, 128, 3, 1, 1, 4, 8, 8), _row(3, 1, 64), None, lambda m: m.d.CS == 64, "the 64-channel ci block"),
    Entry(C(128, 128, 4, 2, 1, 4, 24, 16), _row(4, 2, 128), None, lambda m: (m.d.MH, m.d.MW) == (12, 8), "4x4 stride 2 onto 12x8"),
    Entry(C(64, 128, 4, 2, 1, 3, 32, 64), _row(4, 2, 64), None, lambda m: (m.d.MH, m.d.MW) == (16, 32) and m.nsplit > 1, "4x4 stride 2 onto 16x32"),
    Entry(C(128, 128, 3, 1, 1, 4, 4, 4, up=True), _row(3, 1, 128), None, lambda m: m.d.src_shift == 1 and _declines(m, "up", "tile"),
          "src_shift 1: the up kernel declines (SW % 16)"),
]

# upsample kernel (conv_wgrad_up.hip) and what it declines: bf16 and f16
UP = [
    Entry(C(64, 32, 3, 1, 1, 2, 8, 16, up=True), "wgrad_up_kernel<2, true>", None, lambda m: m.ntiles == 2, "8 x 16 low-res tiles, Cout 32"),
    Entry(C(64, 32, 3, 1, 1, 1, 4, 32, up=True), "wgrad_up_kernel<2, false>", None, lambda m: m.ntiles == 1, "one tile per image"),
    Entry(C(128, 64, 3, 1, 1, 1, 12, 32, up=True), "wgrad_up_kernel<4, false>", None, lambda m: (m.tiles_y, m.ny) == (3, 2),
          "three tile rows, two ci blocks"),
    Entry(C(64, 128, 3, 1, 1, 2, 8, 48, up=True), "wgrad_up_kernel<4, true>", None, lambda m: (m.tiles_x, m.nz) == (3, 2),
          "three 16-wide tile columns"),
    Entry(C(64, 32, 3, 1, 1, 2, 6, 32, up=True), _k((32, 64, 1, 4, 32)), None,
          lambda m: _declines(m, "up", "tile", "row") and m.d.src_shift == 1 and m.branch == "CDw%32" and m.d.P > 1024,
          "split-K with src_shift 1: up declines on SH % 4, tile on MH % 8"),
    Entry(C(32, 32, 3, 1, 1, 2, 8, 16, up=True), _tile(2, 2, 256, 1, 9, 2), None, lambda m: _declines(m, "up") and m.d.src_shift == 1,
          "tile kernel with src_shift 1: up declines on CS % 64"),
    # not in the issue's tables: the two other tile forms a layer through the upsample reaches
    Entry(C(32, 64, 3, 1, 1, 2, 8, 16, up=True), _rr(4, 2, 4), None, lambda m: _declines(m, "up") and m.d.src_shift == 1 and m.tiles_y == 2,
          "row-reuse tile kernel with src_shift 1: up declines on CS % 64"),
    Entry(C(128, 128, 3, 1, 1, 2, 8, 8, up=True), _tile(4, 4, 512, 1, 9, 4, ", false, true"), None,
          lambda m: _declines(m, "up") and m.d.src_shift == 1 and (m.TH, m.TW) == (16, 16) and (m.ny, m.nz) == (2, 2),
          "16 x 16 tiles with src_shift 1: up declines on SW % 16"),
]

H16 = ("bf16", "f16")
TABLES = [("splitk", SPLITK, MODES), ("tile", TILE, H16), ("row", ROW, H16), ("up", UP, H16)]


def expected_kernel(e, mode):
    return e.kernel32 if mode == "fp32" else e.kernel


def all_runs():
    """[(table, entry, mode)] for every case and every mode it runs in"""
    return [(t, e, mode) for t, es, modes in TABLES for e in es for mode in modes]


# class III: one case per kernel family and mode
CLASS3 = [(SPLITK[4], MODES), (TILE[1], H16), (TILE[11], H16), (ROW[1], H16), (UP[2], H16)]
