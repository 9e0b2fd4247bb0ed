"""f64 references, a model of the launch geometry and the case tables for the kernels of csrc/pointwise.hip (a helper, not a test;
imports torch only and runs without a GPU).

References.  Every operand is first rounded to the storage format of the mode (`rt`), then held in f64; every reference is plain
f64 torch on those values, gradients from closed forms (tests/test_pointwise_cpu.py holds them against f64 autograd).  Beside each
value a reference returns the magnitude `A` of the expression it came from: the same expression with every term replaced by its
absolute value (A >= |value|), which is what an evaluation in f32 loses precision against.

Bounds (derived, none of them a fraction of max|ref|).  u_fmt = unit roundoff of the stored format, e = 2^-24:
  element-wise   |got - ref| <= 1.01 u_fmt |ref| + 8 e A          one rounding to storage + the f32 arithmetic of <= 8 operations
  reductions     |got - ref| <= g(depth + ops) S + slack          g(k) = k e / (1 - k e), the bound of recursive summation;
                 depth = additions on the longest path (thread loop, wave / LDS sum, atomics) read off the kernel for the case's
                 geometry, S = sum of the terms' magnitudes A, ops = f32 roundings that form ONE term (0 where a term is a product
                 of two 16-bit operands, which is exact in f32)
  slack          where a kernel rounds an f32 value to the storage format and goes on computing with the ROUNDED value (the dot
                 against the recomputed y, the 2x2 pool of the stored dx), the f32 value may sit on the other side of a rounding
                 boundary than the f64 one: slack = sum |weight| |round(v + 8 e A) - round(v - 8 e A)|, exactly what those elements
                 can move the result by (zero for nearly all of them).
LeakyReLU kinks: inputs are built (`fix_kinks`) so that no pre-activation lies within KINK = 1e-3 of zero, ~10^4 x the f32 evaluation
error at these magnitudes; the references assert it.

Geometry.  `nblocks`, `sblocks`, `affine_grid` (+ the launcher's pooling fix-up), the grids of xmc_colsum and the two branches of
xmc_global_avgpool are restated here as integer arithmetic; every case of the tables carries the regime it is there for as a
predicate on that model, and tests/test_pointwise_cpu.py asserts each predicate."""
import zlib

import torch

NT, UN, STREAM_BLOCKS = 256, 4, 1024
E32 = 2.0 ** -24
U_FMT = {"fp32": 2.0 ** -24, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}
DTYPE = {"fp32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
MODES = ("fp32", "bf16", "f16")
SLOPE = float(torch.tensor(0.2, dtype=torch.float32))       # XMC_LRELU = 0.2f, as the kernels hold it
KINK = 1e-3
TANH_ABS = 1e-7                                              # common.h: tanh_fast's documented absolute error


# ------------------------------------------------------------------------------------------ formats, inputs
def rt(t, mode):
    """round to the storage format of `mode` (through f32, as the device does), back in f64"""
    return t.float().to(DTYPE[mode]).double()


def randn(gen, shape, mode, scale=1.0, device=None):
    """drawn on the host (the same values everywhere), rounded and kept on `device`: the large cases hold their f64 reference there"""
    return rt((torch.randn(shape, generator=gen) * scale).to(device), mode)


def rand_f32(gen, shape, scale=1.0, shift=0.0, device=None):
    """f32 parameters (never stored in 16 bits), in f64"""
    return (torch.randn(shape, generator=gen) * scale + shift).float().to(device).double()


def fix_kinks(x, pre, mode):
    """move the elements of x whose pre-activations (`pre(x)` -> tensors shaped like x) lie within KINK of zero by +0.25, re-round, repeat"""
    for _ in range(64):
        bad = torch.zeros_like(x, dtype=torch.bool)
        for p in pre(x):
            bad |= p.abs() < KINK
        if not bad.any():
            return x
        x = rt(torch.where(bad, x + 0.25, x), mode)
    raise AssertionError("fix_kinks did not converge")


def gen_for(*key):
    """a generator seeded by the case, the same on every machine"""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def kinkfree(gen, shape, mode, device=None):
    return fix_kinks(randn(gen, shape, mode, device=device), lambda t: (t,), mode)


def min_abs(*ts):
    return min(float(t.abs().min()) for t in ts)


# ------------------------------------------------------------------------------------------ bounds
HALF_SUBNORMAL_STEP = {"fp32": 2.0 ** -150, "bf16": 2.0 ** -134, "f16": 2.0 ** -25}      # rounding below the format's normal range


def elem_bound(ref, A, mode, extra_abs=0.0):
    return 1.01 * U_FMT[mode] * ref.abs() + 8 * E32 * A + HALF_SUBNORMAL_STEP[mode] + extra_abs


def gamma(k):
    return k * E32 / (1.0 - k * E32)


def red_bound(S, depth, ops=0, slack=0.0):
    return gamma(depth + ops) * S + slack


def flip_slack(v, A, weight, mode):
    """what rounding v to the format on the other side of a boundary can move sum(weight * round(v)) by, element by element"""
    d = 8 * E32 * A
    return weight.abs() * (rt(v + d, mode) - rt(v - d, mode)).abs()


# ------------------------------------------------------------------------------------------ launch geometry (pointwise.hip, restated)
def cdiv(a, b):
    return -(-a // b)


def nblocks(items, per_block=NT, cap=256 * 16):
    return min(max(cdiv(items, per_block), 1), cap)


def sblocks(n8):
    return nblocks(cdiv(n8, UN), NT, STREAM_BLOCKS)


def stream_geom(n8):
    """map1 / map2 / signmask / scale_mask_dot: a workgroup walks NT*UN consecutive vectors per lap"""
    grid = sblocks(n8)
    return dict(grid=grid, laps=cdiv(n8, grid * NT * UN), last_block_vectors=n8 - (cdiv(n8, NT * UN) - 1) * NT * UN,
                depth=8 * UN * cdiv(n8, grid * NT * UN) + 6 + NT // 64 + grid)


def stride_geom(total, cap=256 * 16, adds_per_item=8):
    """one item per thread per lap of a grid-stride loop; depth: thread loop + wave_sum + the block's waves + one atomic per block"""
    grid = nblocks(total, NT, cap)
    laps = cdiv(total, grid * NT)
    return dict(grid=grid, laps=laps, depth=adds_per_item * laps + 6 + NT // 64 + grid)


def affine_grid(HW, C8, N, ppl):
    groups = NT // C8
    while ppl > 4 and N * cdiv(HW, groups * ppl) < 256:
        ppl >>= 1
    bx = max(cdiv(HW, groups * ppl), 1)
    return dict(groups=groups, ppl=ppl, bx=bx, ppb=cdiv(HW, bx))


def affine_fwd_geom(N, H, W, C):
    g = affine_grid(H * W, C // 8, N, 16)
    g["HW"] = H * W
    return g


def affine_bwd_geom(N, H, W, C, pool=False):
    """xmc_affine2_act_bwd: loop units are pixels, or vertical pixel pairs when pooling; per-lane counts by walking the loops"""
    C8 = C // 8
    HW = (H // 2) * W if pool else H * W
    g = affine_grid(HW, C8, N, 32 if pool else 64)
    g["ppb_raw"] = g["ppb"]
    if pool and g["ppb"] & 1:
        g["ppb"] += 1
        g["bx"] = cdiv(HW, g["ppb"])
    groups, ppb, bx = g["groups"], g["ppb"], g["bx"]
    steps_with_second = steps_without_second = max_units = 0
    for b in range(bx):
        p0, p_end = b * ppb, min(HW, (b + 1) * ppb)
        for lane in range(groups):
            p, units = p0 + lane, 0
            while p < p_end:
                second = not pool and p + groups < p_end
                steps_with_second += second
                steps_without_second += not second
                units += 2 if second else 1
                p += groups if pool else 2 * groups
            max_units = max(max_units, units)
    pix = max_units * (2 if pool else 1)                      # pixels summed by one lane
    g.update(HW=HW, C8=C8, last_block=HW - (bx - 1) * ppb, steps_with_second=steps_with_second,
             steps_without_second=steps_without_second, lane_pixels=pix,
             depth_param=pix + groups + bx,                   # thread loop + LDS sum over the lanes + one atomic per pixel block
             depth_dot=8 * pix + 6 + (NT // 64) * N * bx + 1)   # ... wave_sum, one atomic per wave of the launch, the pre-filled value
    return g


def colsum_geom(rows, C):
    C8 = C // 8
    groups_host = 1 if C8 >= NT else NT // C8
    gx, gy = nblocks(rows, groups_host * 8, 1024), cdiv(C8, NT)
    ys = []
    for y in range(gy):
        c8_here = min(C8 - y * NT, NT)
        groups = NT // c8_here
        step = gx * groups
        n_max, n_min = cdiv(rows, step), rows // step           # rows summed by the first / the last row lane
        ys.append(dict(c8_here=c8_here, groups=groups, step=step, idle_threads=NT - groups * c8_here, n_max=n_max, n_min=n_min,
                       unrolled=any(n // 4 for n in (n_max, n_min)), remainder=any(n % 4 for n in (n_max, n_min)),
                       depth=n_max + groups + gx + 1))
    return dict(C8=C8, groups_host=groups_host, gx=gx, gy=gy, ys=ys, depth=max(y["depth"] for y in ys))


def gap_geom(N, HW, C, out_f32=True):
    C8 = C // 8
    if HW >= 256 and out_f32 and C8 <= NT:
        groups = NT // C8
        ppb = max(cdiv(N * HW, 2048), 4 * groups)
        bx = cdiv(HW, ppb)
        return dict(branch="big", groups=groups, ppb=ppb, bx=bx, depth=cdiv(ppb, groups) + groups + bx)
    return dict(branch="small", grid=nblocks(N * C8), depth=HW)


def hinge_depth(n):
    return cdiv(n, NT) + 6 + NT // 64


# ------------------------------------------------------------------------------------------ case tables
FLAT_SMALL = (8, 8 * 1023, 8 * 1025)
FLAT_BIG = 8 * (1024 * 1024 + 1024 + 3)
FLAT_REGIMES = {
    8: ("one vector", lambda n8: n8 == 1),
    8 * 1023: ("UN tail inside the only block", lambda n8: sblocks(n8) == 1 and (UN - 1) * NT < n8 < UN * NT),
    8 * 1025: ("second block with one live vector", lambda n8: sblocks(n8) == 2 and stream_geom(n8)["last_block_vectors"] == 1),
    FLAT_BIG: ("second lap of every grid-stride loop of the family, partial tail",
               lambda n8: stream_geom(n8)["laps"] == 2 and stride_geom(n8, 512)["laps"] >= 2 and stride_geom(n8)["laps"] == 2
               and n8 % NT != 0 and n8 % (NT * UN) != 0),
}

COLSUM_CASES = {
    (1, 8): ("C8 = 1, 256 row lanes, one row", lambda g: g["C8"] == 1 and g["ys"][0]["groups"] == NT and g["ys"][0]["n_max"] == 1),
    (37, 24): ("C8 = 3 does not divide NT, idle thread", lambda g: g["ys"][0]["idle_threads"] > 0),
    (5000, 40): ("unrolled-by-4 loop and remainder both run", lambda g: g["ys"][0]["unrolled"] and g["ys"][0]["remainder"]),
    (300, 4096): ("two blockIdx.y groups", lambda g: g["gy"] == 2 and all(y["c8_here"] == NT for y in g["ys"])),
    (64, 2056): ("last group has c8_here = 1: the kernel's groups differ from the launcher's",
                 lambda g: g["ys"][-1]["c8_here"] == 1 and g["ys"][-1]["groups"] != g["groups_host"]),
    (9001, 2048): ("the 1024-block cap", lambda g: g["gx"] == 1024 and cdiv(9001, g["groups_host"] * 8) > 1024),
}

# (N, H, W, C) of the LOW-resolution side
RESAMPLE_SMALL = (2, 6, 10, 24)
RESAMPLE_BIG = (3, 40, 56, 320)         # its high-resolution side: second lap of up2 / axpby_up / gap_bwd / plain axpby_bwd
RESAMPLE_BIG2 = (3, 80, 112, 320)       # as the pooled OUTPUT: second lap of pool2 (cap 4096 blocks); bf16 only
RESAMPLE_UPBWD = (3, 40, 56, 640)       # second lap of axpby_bwd with up, which walks low-resolution positions (cap 2048 blocks); bf16 only


def resample_regimes():
    def vec(s, up=1):
        return s[0] * s[1] * up * s[2] * up * s[3] // 8
    return [
        ("small: one lap everywhere, C8 = 3 no power of two, W != H",
         stride_geom(vec(RESAMPLE_SMALL, 2))["laps"] == 1 and RESAMPLE_SMALL[1] != RESAMPLE_SMALL[2]),
        ("big: second lap of the loops over high-resolution vectors (cap 4096 blocks)", stride_geom(vec(RESAMPLE_BIG, 2))["laps"] == 2),
        ("big: second lap of plain axpby_bwd (cap 2048 blocks)", stride_geom(vec(RESAMPLE_BIG, 2), 2048)["laps"] >= 2),
        ("big: loops over low-resolution vectors still take one lap (hence big2)",
         stride_geom(vec(RESAMPLE_BIG))["laps"] == 1 and stride_geom(vec(RESAMPLE_BIG), 2048)["laps"] == 1),
        ("big2: second lap of pool2", stride_geom(vec(RESAMPLE_BIG2))["laps"] == 2),
        ("upbwd: second lap of axpby_bwd with up", stride_geom(vec(RESAMPLE_UPBWD), 2048, 32)["laps"] == 2),
        ("big: global_avgpool takes the large-map branch, small: the one-thread-per-chunk branch",
         gap_geom(RESAMPLE_BIG[0], RESAMPLE_BIG[1] * RESAMPLE_BIG[2], RESAMPLE_BIG[3])["branch"] == "big"
         and gap_geom(RESAMPLE_SMALL[0], RESAMPLE_SMALL[1] * RESAMPLE_SMALL[2], RESAMPLE_SMALL[3])["branch"] == "small"),
    ]


CONVERT_SMALL = [(2, c, 5, 7) for c in range(1, 9)]      # (N, C, H, W)
CONVERT_BIG = (5, 3, 512, 416)
HINGE_N = (1, 7, 256, 257, 1000)

# affine pair, no pooling: (N, H, W, C) -> (regime, predicate on affine_bwd_geom)
AFFINE_CASES = {
    (3, 6, 6, 24): ("the anchor: one workgroup per image, at most one pixel per lane",
                    lambda g: g["bx"] == 1 and g["steps_with_second"] == 0 and g["HW"] <= g["groups"]),
    (2, 5, 9, 8): ("C8 = 1: 256 pixel lanes, HW = 45 < groups", lambda g: g["C8"] == 1 and g["groups"] == NT and g["HW"] < g["groups"]),
    (2, 3, 5, 2048): ("C8 = NT: groups = 1, bx > 1, odd pixel count: the last lane step has no second pixel",
                      lambda g: g["C8"] == NT and g["groups"] == 1 and g["bx"] > 1 and g["HW"] % 2 == 1 and g["last_block"] % 2 == 1
                      and g["steps_with_second"] > 0 and g["steps_without_second"] > 0),
    # the issue's (2, 48, 40, 64) has HW = 1920 = 15 * 128: a multiple of ppb.  1900 = 50 * 38 keeps bx = 15 and ppl = 4 with ppb = 127
    (2, 50, 38, 64): ("ppl halved to 4, bx = 15, HW not a multiple of ppb",
                      lambda g: g["ppl"] == 4 and g["bx"] == 15 and g["HW"] % g["ppb"] != 0 and g["last_block"] < g["ppb"]),
    (256, 5, 8, 64): ("ppl stays 64; lanes g < 8 take a second pixel, the others do not",
                      lambda g: g["ppl"] == 64 and g["bx"] == 1 and g["steps_with_second"] == 8 and g["steps_without_second"] == 24),
}
AFFINE_CROSS = ((3, 6, 6, 24), (2, 50, 38, 64))           # every subset of {second affine, dx_in, alpha/dot}
AFFINE_BIG = (32, 41, 50, 512)
AFFINE_BIG_REGIME = ("ppl = 64 with bx > 1 and a partial last block",
                     lambda g: g["ppl"] == 64 and g["bx"] > 1 and g["last_block"] < g["ppb"] and g["steps_with_second"] > 0)

AFFINE_POOL_CASES = {(2, 8, 12, c): ("C8 = %d: the lane exchange at distance C8, W/2 = 6 even" % (c // 8),
                                     lambda g, c=c: g["C8"] == c // 8 and g["C8"] in (1, 2, 4, 8, 16, 32))
                     for c in (8, 16, 32, 64, 128, 256)}
AFFINE_POOL_CASES.update({
    (2, 8, 10, 64): ("W/2 = 5 odd", lambda g: g["C8"] == 8),
    # the issue's (3, 10, 6, 64) has 30 pairs in ONE block (ppb = 30, even).  130 = 5 * 26 pairs: two blocks of 65 before the fix-up
    (3, 10, 26, 64): ("ppb is odd before the launcher's fix-up", lambda g: g["ppb_raw"] % 2 == 1 and g["ppb"] == g["ppb_raw"] + 1 and g["bx"] > 1),
    (2, 64, 64, 32): ("bx > 1: pairs at a block boundary", lambda g: g["bx"] > 1 and g["ppb"] % 2 == 0),
})
AFFINE_POOL_CROSS = ((3, 10, 26, 64), (2, 64, 64, 32))
AFFINE_POOL_REFUSED = ((2, 5, 8, 64), (2, 8, 5, 64), (2, 8, 8, 24), (2, 8, 8, 512))      # odd H, odd W, C8 = 3, C8 = 64


# ------------------------------------------------------------------------------------------ references: flat maps
def lrelu_ref(x, slope=SLOPE):
    assert min_abs(x) >= KINK
    y = torch.where(x > 0, x, slope * x)
    return y, y.abs()


def mask_ref(dy, ref, slope=SLOPE):
    assert min_abs(ref) >= KINK
    y = torch.where(ref > 0, dy, slope * dy)
    return y, y.abs()


def tanh_bwd_ref(dy, y):
    return dy * (1 - y * y), dy.abs() * (1 + y * y)


def axpby_ref(a, b, al):
    return a + al * b, a.abs() + (al * b).abs()


def dot_ref(a, b):
    return float((a * b).sum()), float((a * b).abs().sum())


def scale_mask_dot_ref(dy, ref, al):
    assert min_abs(ref) >= KINK
    g = al * dy * torch.where(ref > 0, 1.0, SLOPE)
    return g, g.abs(), float((dy * ref).sum()), float((dy * ref).abs().sum())


# ------------------------------------------------------------------------------------------ references: pooling / resampling (NHWC)
def sumpool2_ref(x, scale):
    N, H, W, C = x.shape
    q = x.view(N, H // 2, 2, W // 2, 2, C)
    return scale * q.sum((2, 4)), abs(scale) * q.abs().sum((2, 4))


def up2_ref(x):
    return x.repeat_interleave(2, 1).repeat_interleave(2, 2)


def axpby_up_ref(a, b, al, lrelu):
    y, A = axpby_ref(up2_ref(a), b, al)
    if lrelu:
        assert min_abs(y) >= KINK
        s = torch.where(y > 0, 1.0, SLOPE)
        y, A = y * s, A * s
    return y, A


def axpby_bwd_ref(dy, b, al, up, ymask):
    """-> da, A_da (None where the kernel writes none), db, A_db, dalpha, S"""
    if ymask is not None:
        assert min_abs(ymask) >= KINK
        dy = dy * torch.where(ymask > 0, 1.0, SLOPE)
    da = A_da = None
    if up:
        da, A_da = sumpool2_ref(dy, 1.0)
    elif ymask is not None:
        da, A_da = dy, dy.abs()
    return da, A_da, al * dy, (al * dy).abs(), float((dy * b).sum()), float((dy * b).abs().sum())


def gap_ref(x):
    N, H, W, C = x.shape
    return x.view(N, H * W, C).mean(1), x.view(N, H * W, C).abs().mean(1)


def gap_bwd_ref(dy, H, W):
    g = (dy / (H * W))[:, None, None, :].expand(-1, H, W, -1)
    return g, g.abs()


def hinge_ref(v, sign):
    """v f64 [n] -> loss, S, the gradient of v for d loss = 1"""
    t = torch.clamp(1 + sign * v, min=0)
    return float(t.mean()), float(t.mean()), (1 + sign * v > 0).double() * (sign / v.numel())


AL = float(torch.tensor(0.37, dtype=torch.float32))


def flat_case(n, mode, device=None):
    """x, ref: kink-free; dy, b: free; y: a tanh output"""
    g = gen_for("flat", n, mode)
    return dict(x=kinkfree(g, (n,), mode, device), ref=kinkfree(g, (n,), mode, device), dy=randn(g, (n,), mode, device=device),
                b=randn(g, (n,), mode, device=device), y=rt(torch.tanh(torch.randn((n,), generator=g).to(device).double()), mode))


def resample_case(lo, mode, want=("a", "b", "dy", "ymask"), device=None):
    """a [lo], b / dy / ymask [hi]: up2(a) + AL * b and ymask are kink-free"""
    N, H, W, C = lo
    hi = (N, 2 * H, 2 * W, C)
    g = gen_for("resample", lo, mode)
    c = dict(a=randn(g, lo, mode, device=device))
    if "b" in want:
        up = up2_ref(c["a"])
        c["b"] = fix_kinks(randn(g, hi, mode, device=device), lambda t: (up + AL * t,), mode)
    if "dy" in want:
        c["dy"] = randn(g, hi, mode, device=device)
    if "ymask" in want:
        c["ymask"] = kinkfree(g, hi, mode, device)
    return c


def hinge_case(n, mode):
    """logits with no 1 + sign * v within KINK of zero, for either sign"""
    return fix_kinks(randn(gen_for("hinge", n, mode), (n,), mode, 1.5), lambda t: (1 - t.abs(),), mode)


def affine_case(shape, mode, two=True, slope=SLOPE, device=None):
    return affine_inputs(gen_for("affine", shape, mode, two, slope), shape, mode, two, slope, device)


# ------------------------------------------------------------------------------------------ reference: the affine pair
def affine_inputs(gen, shape, mode, two=True, slope=SLOPE, device=None):
    """x (kink-free), the [N,C] parameters drawn per (n, c), dy, dx_in"""
    N, H, W, C = shape
    ps = [rand_f32(gen, (N, C), 0.5, sh, device) for sh in (1.0, 0.0, -1.0, 0.0)]
    ps = ps if two else ps[:2]
    x = fix_kinks(randn(gen, shape, mode, device=device), lambda t: affine_pre(t, ps, slope), mode)
    return x, ps, randn(gen, shape, mode, device=device), randn(gen, shape, mode, device=device)


def _e(t):
    return t[:, None, None, :]


def affine_pre(x, ps, slope=SLOPE):
    u = x * _e(ps[0]) + _e(ps[1])
    if len(ps) == 2:
        return (u,)
    return u, torch.where(u > 0, u, slope * u) * _e(ps[2]) + _e(ps[3])


def affine_ref(x, ps, mode, dy=None, dx_in=None, alpha=None, pool=False, slope=SLOPE):
    """lrelu(lrelu(x g0 + b0) g1 + b1) (one affine with len(ps) == 2) and its backward -> dict:
    y, A_y; dx, A_dx; grads [(value [N,C], S [N,C])] in the order of ps; dot, S_dot, slack_dot (with alpha); pool, A_pool, slack_pool"""
    two = len(ps) == 4
    g0, b0 = _e(ps[0]), _e(ps[1])
    u = x * g0 + b0
    su = torch.where(u > 0, 1.0, slope)
    a1, A_a1 = u * su, ((x * g0).abs() + b0.abs()) * su
    if two:
        g1, b1 = _e(ps[2]), _e(ps[3])
        v = a1 * g1 + b1
        sv = torch.where(v > 0, 1.0, slope)
        y, A_y = v * sv, (A_a1 * g1.abs() + b1.abs()) * sv
        kink = min_abs(u, v)
    else:
        g1, sv, y, A_y, kink = 1.0, 1.0, a1, A_a1, min_abs(u)
    assert kink >= KINK, kink
    out = dict(y=y, A_y=A_y, kink=kink)
    if dy is None:
        return out
    dvv = dy * (1.0 if alpha is None else alpha) * sv
    du = dvv * g1 * su
    dx = du * g0
    A_dx = dx.abs()
    if dx_in is not None:
        dx, A_dx = dx + dx_in, A_dx + dx_in.abs()
    red = lambda t: t.sum((1, 2))
    grads = [(red(du * x), red((du * x).abs())), (red(du), red(du.abs()))]
    if two:
        grads += [(red(dvv * a1), red(dvv.abs() * A_a1)), (red(dvv), red(dvv.abs()))]
    out.update(dx=dx, A_dx=A_dx, grads=grads)
    if alpha is not None:
        yr = rt(y, mode)
        out.update(dot=float((dy * yr).sum()), S_dot=float((dy.abs() * A_y).sum()), slack_dot=float(flip_slack(y, A_y, dy, mode).sum()))
    if pool:
        dxr = rt(dx, mode)
        p, A_p = sumpool2_ref(dxr, 1.0)
        sl, _ = sumpool2_ref(flip_slack(dx, A_dx, torch.ones((), device=dx.device), mode), 1.0)
        out.update(pool=p, A_pool=A_p, slack_pool=sl)
    return out


AFFINE_GRAD_OPS = 8          # f32 roundings that form one term of dg0 / db0 / dg1 / db1 (alpha, two slopes, g1, the recomputed a1, the product)
