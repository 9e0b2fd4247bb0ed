"""DiffAugment on the GPU: the kernels of csrc/augment.hip against the f64 restatement (tests/diffaug_ref.py), the autograd nodes (first and
second order), the wiring through the discriminator and `gan_iteration`, and the entry point's ``--diffaug``.

Error bar of the kernel tests (derived, not tuned).  Per element
    |err| <= u16 |ref| + 2^-24 (16 + n_img) A,      A = (max|x| + |b|) (|s| + |1-s|) (|c| + |1-c|)
u16: unit roundoff of the output format as the tests take it (2^-8 bf16, 2^-11 IEEE half, 0 f32: the one rounding at the store);
n_img = C*H*W: the worst case of an f32 sum of that many terms in any order (the image mean); 16: the dozen f32 operations per element,
each rounding a quantity of magnitude <= A.  The transposed map has no b-term: there A = max|dy| (|s| + |1-s|) (|c| + |1-c|)."""
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diffaug_ref as R
import xmc_ref as X
from golden_util import CFG_DIR
from parity_util import DEV, build_product, setup_cfg
from xmc_gan_amd import lib as L
from xmc_gan_amd import ops
from xmc_gan_amd.augment import DiffAugment

MODES = ["fp32", "bf16", "f16"]
SHAPES = [(3, 8, 8), (2, 16, 12), (2, 64, 64)]       # the second catches swapped axes, the third is more than one workgroup per image
U16 = {"fp32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}
C = 3
EPS = 2.0 ** -24


@pytest.fixture(autouse=True)
def _restore_precision():
    yield
    ops.set_precision("bf16")


# ----------------------------------------------------------------------------------------------------------- inputs
def _cases(N, H, W):
    """[(cut, rows f64 [N,8])]: hand-picked rows in batches of N.  Largest shifts of both signs, shifts by the whole width / height, the cutout
    square over each corner, over (almost) the whole image and over all of it, contrast / saturation / brightness alone, the identity."""
    rw, rh, c = int(W * 0.125 + 0.5), int(H * 0.125 + 0.5), int(min(H, W) * 0.5 + 0.5)
    h2, big = c // 2, max(H, W)
    groups = [
        (c, [[0.3, 0.4, 1.3, rw, rh, 1, 1], [-0.2, 1.7, 0.6, -rw, -rh, H - c - 1, W - c - 1],
             [0.1, 0.8, 1.2, W, 0, 2, 2], [0.1, 0.8, 1.2, -W, 1, 2, 2], [-0.4, 1.9, 0.5, 0, H, 0, 0],
             [0.2, 0.0, 1.5, 0, 0, -h2, -h2], [0.0, 2.0, 0.5, 1, 0, -h2, W - h2],
             [-0.5, 1.0, 1.0, 0, -1, H - h2, -h2], [0.5, 0.5, 1.0, -1, 1, H - h2, W - h2]]),
        (big, [[0.25, 0.5, 0.75, 1, -1, 0, 0], [0.25, 0.5, 0.75, 0, 0, -1, -1], [0.0, 1.0, 1.0, 0, 0, 1, 0]]),
        (0, [[0.0, 1.0, 0.7, 0, 0, 0, 0], [0.0, 0.3, 1.0, 0, 0, 0, 0], [0.4, 1.0, 1.0, 0, 0, 0, 0], [0.0, 1.0, 1.0, 0, 0, 0, 0]]),
    ]
    out = []
    for cut, rows in groups:
        for i in range(0, len(rows), N):
            chunk = [rows[(i + k) % len(rows)] + [0.0] for k in range(N)]
            out.append((cut, torch.tensor(chunk, dtype=torch.float64)))
    return out


def _img8(N, H, W, dtype, gen, pad_noise=False):
    """[N,H,W,8] with C real channels, generated in `dtype`; pad channels zero (an image) or arbitrary (an incoming gradient)"""
    x = torch.zeros(N, H, W, 8)
    x[..., :C] = torch.rand(N, H, W, C, generator=gen) * 2 - 1
    if pad_noise:
        x[..., C:] = torch.rand(N, H, W, 8 - C, generator=gen)
    return x.to(dtype).to(DEV)


def _nchw(x8):
    return x8.detach()[..., :C].permute(0, 3, 1, 2).double().cpu()


def _amp(P):
    return R.amplification(torch.cat((torch.zeros_like(P[:, :1]), P[:, 1:]), 1), 1.0)       # (|s| + |1-s|)(|c| + |1-c|) per image


@functools.lru_cache(maxsize=None)
def _run(mode, shape):
    """forward and transposed kernels on every case of a shape, once per (mode, shape): shared by the tests below"""
    ops.set_precision(mode)
    N, H, W = shape
    gen = torch.Generator().manual_seed(1000 * H + W)
    res = []
    for cut, P in _cases(N, H, W):
        x = _img8(N, H, W, ops.act_dtype(), gen).requires_grad_()
        dy = _img8(N, H, W, ops.act_dtype(), gen, pad_noise=True)
        Pd = P.float().to(DEV)
        y = ops.diffaug(x, Pd, cut)
        (dx,) = torch.autograd.grad(y, x, dy)
        torch.cuda.synchronize()
        res.append(dict(cut=cut, P=P, x=x.detach().cpu(), dy=dy.cpu(), y=y.detach().cpu(), dx=dx.cpu()))
    return res


# ----------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_forward_and_transposed_against_the_restatement(mode, shape):
    """y = A x + b-term and dx = A^T dy, element by element, within the derived bar of the module docstring."""
    N, H, W = shape
    worst = [0.0, 0.0]
    for r in _run(mode, shape):
        x, dy, P, cut = _nchw(r["x"]), _nchw(r["dy"]), r["P"], r["cut"]
        ref = R.forward(x, P, cut)
        bnd = R.bound(ref, P, x.abs().max().item(), U16[mode], C * H * W)
        frac = ((_nchw(r["y"]) - ref).abs() / bnd).max().item()
        ref_t = R.transpose(dy, P, cut)
        P0 = P.clone()
        P0[:, 0] = 0
        bnd_t = R.bound(ref_t, P0, dy.abs().max().item(), U16[mode], C * H * W)
        frac_t = ((_nchw(r["dx"]) - ref_t).abs() / bnd_t).max().item()
        print(f"  [{mode} {shape} cut {cut}] fraction of the bound used: forward {frac:.3f}, transposed {frac_t:.3f}")
        worst = [max(worst[0], frac), max(worst[1], frac_t)]
        assert frac <= 1.0 and frac_t <= 1.0, (mode, shape, cut, frac, frac_t)
    print(f"\n[diffaug kernels, {mode}, {shape}] worst fraction of the bound used: forward {worst[0]:.3f}, transposed {worst[1]:.3f}")


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_exact_zeros_and_exact_identity(mode, shape):
    """pad channels exactly 0 in output and gradient; cut and out-of-frame pixels exactly 0 in the output; identity rows reproduce their image
    bit for bit (all 8 channels)."""
    N, H, W = shape
    seen_identity = seen_dead = 0
    for r in _run(mode, shape):
        P, cut, y, dx, x = r["P"], r["cut"], r["y"], r["dx"], r["x"]
        assert (y[..., C:] == 0).all() and (dx[..., C:] == 0).all()
        keep, _, _ = R._geometry(P, H, W, cut)
        assert (y[~keep] == 0).all()
        seen_dead += int((~keep).sum())
        for n in range(N):
            if cut == 0 and P[n, :5].tolist() == [0.0, 1.0, 1.0, 0.0, 0.0]:
                assert torch.equal(y[n], x[n]), (mode, shape, n)
                seen_identity += 1
    assert seen_identity >= 1 and seen_dead > 0


@pytest.mark.parametrize("shape", SHAPES)
def test_adjoint_identity_fp32(shape):
    """<A x, g> and <x, A^T g>, both accumulated in f64 from the kernels' outputs, per image within 2^-24 (16 + n_img) (|s|+|1-s|)(|c|+|1-c|)
    sum|x||g|: the bound of the module docstring with the magnitudes of the inner product's terms in place of max|x|."""
    ops.set_precision("fp32")
    N, H, W = shape
    gen = torch.Generator().manual_seed(5)
    worst = 0.0
    for cut, P in _cases(N, H, W):
        x, g = _img8(N, H, W, torch.float32, gen), _img8(N, H, W, torch.float32, gen, pad_noise=True)
        Pd = P.float().to(DEV)
        Ax = ops.DiffAugFn.apply(x, Pd, cut, True, C, True)
        ATg = ops.DiffAugBwdFn.apply(g, Pd, cut, True, C)
        lhs = (_nchw(Ax) * _nchw(g)).sum(dim=(1, 2, 3))
        rhs = (_nchw(x) * _nchw(ATg)).sum(dim=(1, 2, 3))
        bnd = EPS * (16 + C * H * W) * _amp(P) * (_nchw(x).abs() * _nchw(g).abs()).sum(dim=(1, 2, 3))
        frac = ((lhs - rhs).abs() / bnd).max().item()
        print(f"  [adjoint {shape} cut {cut}] fraction of the bound used: {frac:.3f}")
        worst = max(worst, frac)
        assert frac <= 1.0, (shape, cut, lhs, rhs, bnd)
    print(f"\n[diffaug adjoint identity, {shape}] worst fraction of the bound used: {worst:.3f}")


@pytest.mark.parametrize("shape", SHAPES)
def test_second_order_the_way_the_gradient_penalty_uses_it_fp32(shape):
    """r = grad(y, x, grad_outputs=w, create_graph=True) is A^T w; sum(r^2).backward() then hands w the gradient 2 A A^T w through the backward
    node's own backward (the forward kernels without the b-term).  Bar: the module docstring's bound applied twice.  With e = 2^-24 (16 + n_img)
    and a = (|s|+|1-s|)(|c|+|1-c|): r carries an error <= e a max|w| and |r| <= a max|w|; A (2 r) adds <= e a 2 max|r| and maps r's error to
    <= 2 a e a max|w|; together 4 e a^2 max|w| per element (second-order terms in e dropped against the slack of 16)."""
    ops.set_precision("fp32")
    N, H, W = shape
    gen = torch.Generator().manual_seed(6)
    worst = 0.0
    for cut, P in _cases(N, H, W):
        x = _img8(N, H, W, torch.float32, gen).requires_grad_()
        w = _img8(N, H, W, torch.float32, gen, pad_noise=True).requires_grad_()
        y = ops.diffaug(x, P.float().to(DEV), cut)
        (r,) = torch.autograd.grad(y, x, grad_outputs=w, create_graph=True)
        (r.float() ** 2).sum().backward()
        ref = 2 * R.linear(R.transpose(_nchw(w), P, cut), P, cut)
        bnd = 4 * EPS * (16 + C * H * W) * (_amp(P) ** 2).view(-1, 1, 1, 1) * _nchw(w).abs().max().item()
        frac = ((_nchw(w.grad) - ref).abs() / bnd).max().item()
        print(f"  [second order {shape} cut {cut}] fraction of the bound used: {frac:.3f}")
        worst = max(worst, frac)
        assert frac <= 1.0, (shape, cut, frac)
        assert (w.grad[..., C:] == 0).all() and x.grad is None
    print(f"\n[diffaug second order, {shape}] worst fraction of the bound used: {worst:.3f}")


class _Count:
    """counts the library calls that go through lib.call, by entry point"""

    def __init__(self, monkeypatch):
        self.n = {}
        orig = L.call

        def call(name, *a):
            self.n[name] = self.n.get(name, 0) + 1
            return orig(name, *a)
        monkeypatch.setattr(L, "call", call)

    def diffaug(self):
        return {k: v for k, v in self.n.items() if k.startswith("xmc_diffaug")}


def test_a_policy_without_colour_never_launches_the_sums_pass(monkeypatch):
    ops.set_precision("bf16")
    N, H, W = 2, 16, 12
    gen = torch.Generator().manual_seed(7)
    cut = 6
    P = torch.tensor([[0, 1, 1, 2, -1, 3, 8, 0], [0, 1, 1, -1, 2, -3, -3, 0]], dtype=torch.float64)
    x = _img8(N, H, W, torch.bfloat16, gen).requires_grad_()
    dy = _img8(N, H, W, torch.bfloat16, gen, pad_noise=True)
    cnt = _Count(monkeypatch)
    y = ops.diffaug(x, P.float().to(DEV), cut, color=False)
    (dx,) = torch.autograd.grad(y, x, dy)
    assert cnt.diffaug() == {"xmc_diffaug_apply": 2}
    # without colour the map only moves and masks values: exact
    assert torch.equal(_nchw(y), R.forward(_nchw(x), P, cut)) and torch.equal(_nchw(dx), R.transpose(_nchw(dy), P, cut))
    # no backward launch for an input that takes no gradient (the discriminator step's detached images)
    y2 = ops.diffaug(x.detach(), P.float().to(DEV), cut, color=False)
    assert not y2.requires_grad and cnt.diffaug() == {"xmc_diffaug_apply": 3}
    # with colour: one sums launch per direction
    y3 = ops.diffaug(x, P.float().to(DEV), cut)
    torch.autograd.grad(y3, x, dy)
    assert cnt.diffaug() == {"xmc_diffaug_apply": 5, "xmc_diffaug_sums": 2}


def test_argument_checks():
    ops.set_precision("fp32")
    x = torch.zeros(1, 4, 4, 8, device=DEV)
    P = DiffAugment.identity_rows(1).to(DEV)
    y = torch.empty_like(x)
    parts = torch.empty(1, L.DIFFAUG_PARTS, device=DEV)
    lib, p, st = L.load(), ops._p, ops._st()
    ok = lambda C_, cut, dt: lib.xmc_diffaug_apply(p(x), p(P), None, p(y), 1, 4, 4, C_, cut, 0, 0, dt, st)
    assert ok(3, 0, L.F32) == 0 and ok(8, 2, L.F32) == 0 and ok(1, 0, L.F32) == 0
    assert ok(9, 0, L.F32) == -3 and ok(0, 0, L.F32) == -3 and ok(3, -1, L.F32) == -3 and ok(3, 0, 7) == -3
    oks = lambda C_, cut, dt: lib.xmc_diffaug_sums(p(x), p(P), p(parts), 1, 4, 4, C_, cut, 1, dt, st)
    assert oks(3, 0, L.F32) == 0
    assert oks(9, 0, L.F32) == -3 and oks(0, 0, L.F32) == -3 and oks(3, -1, L.F32) == -3 and oks(3, 0, 7) == -3
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------- the discriminator
def _rows_64(n):
    rows = [[0.3, 0.4, 1.3, 8, -5, 10, 40, 0], [-0.2, 1.7, 0.6, -3, 8, -16, 20, 0], [0.1, 0.9, 0.8, 0, 2, 50, -7, 0], [0.0, 1.2, 1.1, -8, -8, 30, 30, 0]]
    return torch.tensor([rows[i % 4] for i in range(n)], dtype=torch.float64)


def test_gradient_through_the_discriminator_fp32():
    """d sum(netD(diffaug(x))) / dx is the discriminator's own gradient at the augmented image pushed through the restatement's transpose;
    bar: the fp32 gradient bar of tests/test_models_gpu.py (5e-3 relative L2)."""
    ops.set_precision("fp32")
    cfg, h = setup_cfg("df_gan_damsm_nomagp.yml", **{"TRAIN.NCH": 8})
    _, netD, _, _ = build_product(h, X.synth_params(X.gen_shapes(h), 5), X.synth_params(X.netd_shapes(h), 6), 1e-3)
    N, S, cut = 2, cfg.IMG.SIZE, 32
    assert S == 64
    gen = torch.Generator().manual_seed(8)
    P = _rows_64(N)
    Pd = P.float().to(DEV)
    x8 = _img8(N, S, S, torch.float32, gen).requires_grad_()
    (got,) = torch.autograd.grad(netD(None, nhwc8=ops.diffaug(x8, Pd, cut)).float().sum(), x8)
    xa = ops.diffaug(x8.detach(), Pd, cut).detach().requires_grad_()
    (ga,) = torch.autograd.grad(netD(None, nhwc8=xa).float().sum(), xa)
    want = R.transpose(_nchw(ga), P, cut)
    err = ((_nchw(got) - want).norm() / want.norm()).item()
    print(f"\n[diffaug through netD, fp32] relative L2 error of d/dx: {err:.2e} (bar 5e-3)")
    assert want.norm().item() > 0 and err <= 5e-3
    assert (got[..., C:] == 0).all()


@pytest.mark.parametrize("route,over,at_the_bar", [
    ("one 2B pass", {}, ()),                                                # real and generated images in one engine-layout buffer
    ("three passes", {"DISC.SPEC_NORM": True}, ("errD_real", "errD_fake", "errD_mismatch", "ds_loss")),      # both in the engine layout, MA-GP under ops.composable()
    ("generated image as NCHW", {"GEN.ENCODER_NAME": "CONCEPT_OUTATTN_GEN"}, ("errD_fake", "fake")),      # a generator without nhwc_out
], ids=["one-2B-pass", "three-passes", "generated-image-as-NCHW"])
def test_identity_rows_through_the_iteration_fp32(route, over, at_the_bar):
    """all-identity rows: the D step's forward-only losses and the generated image are bit-equal to the iteration without the option, the
    losses behind an optimizer step within the fp32 loss bar of tests/test_models_gpu.py (1e-3 relative, 1e-4 absolute).  With MA-GP,
    ENCODER_LOSS.SENT, ENCODER_LOSS.DISC (the generator step's second pass over the real images) and RMIS_LOSS, on each of the three ways an
    image reaches the discriminator.

    ``at_the_bar``: what is not bit-equal on a route, compared at that loss bar instead (per element for the image).  Measured in four runs
    each before and after the iteration was split into phases, with the same figures: under spectral norm any two discriminators built
    from the same weights differ by an ulp or two in their logits, so the three hinge terms differ by 0 .. 2.4e-7 from run to run (ds_loss by 0
    in all eight runs, the image by 0: the generator is not involved); the word-attention generator's image differs by 1.4e-6 .. 2.4e-6
    between any two runs (f32 atomics order of its BatchNorm sums) and errD_fake with it by 2.4e-7 .. 9.5e-7, the quantities that depend on
    the real images alone by 0."""
    import xmc_gan.train_gan as tg
    ops.set_precision("fp32")
    cfg, h = setup_cfg("df_gan_damsm.yml", **{"TRAIN.NCH": 8, **over})
    assert cfg.TRAIN.MAGP and cfg.TRAIN.RMIS_LOSS and cfg.TRAIN.ENCODER_LOSS.SENT and cfg.TRAIN.ENCODER_LOSS.DISC
    b = X.synth_batch(h, 4, seed=500, words_len=cfg.TEXT.MAX_LENGTH)
    batch = [b[k].to(DEV) for k in ("imgs", "sent_embs", "words_embs", "mask", "noise")]
    outs = []
    for with_aug in (False, True):
        netG, netD, optG, optD = build_product(h, X.synth_params(X.gen_shapes(h), 5), X.synth_params(X.netd_shapes(h), 6), 1e-3)
        aug = DiffAugment("color,translation", 4, cfg.IMG.SIZE, cfg.IMG.SIZE, DEV, seed=1) if with_aug else None      # (identity until refresh())
        o = tg.gan_iteration(netG, netD, optG, optD, *batch, {}, tg.StepOptions(diffaug=aug))
        torch.cuda.synchronize()
        outs.append({k: v.float().cpu() for k, v in o.items()})
    plain, ident = outs
    assert set(plain) == set(ident)
    forward_only = ("errD_real", "errD_fake", "errD_mismatch", "ds_loss", "fake")
    print(f"\n  [identity rows, {route}] forward-only differences: " + ", ".join(f"{k} {float((plain[k] - ident[k]).abs().max()):.3g}"
                                                                                for k in forward_only))
    for k in forward_only:
        if k in at_the_bar:
            assert ((ident[k] - plain[k]).abs() <= 1e-3 * plain[k].abs() + 1e-4).all(), (k, plain[k], ident[k])
        else:
            assert torch.equal(plain[k], ident[k]), (k, plain[k], ident[k])
    for k in sorted(set(plain) - set(forward_only)):
        a, r = float(ident[k]), float(plain[k])
        print(f"  [identity rows] {k}: {a:.7g} vs {r:.7g}")
        assert abs(a - r) <= 1e-3 * (6.0 if k == "d_loss_gp" else 1.0) * abs(r) + 1e-4, (k, a, r)


# ----------------------------------------------------------------------------------------------------------- the entry point
def _mini_yml(tmp_path, **subst):
    """df_gan_damsm.yml shrunk for a test run (as tests/test_entrypoint_gpu.py does)"""
    txt = open(os.path.join(CFG_DIR, "df_gan_damsm.yml")).read()
    rep = {"NCH: 32": "NCH: 8", "VOCA_SIZE: 27297": "VOCA_SIZE: 40", "BATCH_SIZE: 88": "BATCH_SIZE: 4", "LOG_INTERVAL: 200": "LOG_INTERVAL: 2",
           "NUM_WORKERS: 8": "NUM_WORKERS: 0", "ENCODER_DIR: data/DAMSMencoders/coco/text_encoder100.pth": "ENCODER_DIR: ''",
           "MAX_LENGTH: 20": "MAX_LENGTH: 8", "MAGP: true": "MAGP: false"}
    rep.update(subst)
    for a, b in rep.items():
        assert a in txt, a
        txt = txt.replace(a, b)
    path = tmp_path / "mini.yml"
    path.write_text(txt)
    return str(path)


def _main(tmp_path, yml, tag, *extra):
    import xmc_gan.train_gan as tg
    last = tg.main(["--cfg", yml, "--synthetic", "6", "--max_epoch", "1", "--precision", "fp32", "--seed", "11", "--output_dir", str(tmp_path / tag),
                    *extra])
    netG, netD = tg.main.last_models
    return last, ({"G." + k: v.detach().float().cpu().clone() for k, v in netG.state_dict().items()} |
                  {"D." + k: v.detach().float().cpu().clone() for k, v in netD.state_dict().items()})


@pytest.mark.parametrize("case", ["headline losses", "MA-GP"])
def test_entry_point_graph_replay_equals_eager_launches_with_diffaug(tmp_path, monkeypatch, case):
    """six iterations of ``--diffaug color,translation,cutout`` through `main()`, replayed as hipGraphs and launched eagerly, from the same seed:
    same final weights and last losses, to the bars of test_entry_point_graph_replay_equals_eager_launches (tests/test_entrypoint_gpu.py; see
    there for their derivation).  The rows are redrawn on the host before every iteration, so equality shows that a replay reads the new rows.
    And the augmentation is in effect: the last errD_fake differs from that of a run without the flag."""
    yml = _mini_yml(tmp_path, **{"MAGP: true": "MAGP: true" if case == "MA-GP" else "MAGP: false"})
    cnt = _Count(monkeypatch)
    res = {g: _main(tmp_path, yml, f"run{g}", "--graph", str(g), "--diffaug", "color,translation,cutout") for g in (1, 0)}
    assert res[1][0].get("hipgraph") is True and "hipgraph" not in res[0][0]
    assert cnt.diffaug().get("xmc_diffaug_apply", 0) > 0 and cnt.diffaug().get("xmc_diffaug_sums", 0) > 0
    worst, flipped = 0.0, 0
    for k, a in res[1][1].items():
        b = res[0][1][k]
        d = (a - b).abs().flatten().double()
        top = d.topk(max(1, d.numel() // 10000)).values
        e = ((d.square().sum() - top.square().sum()).clamp_min(0).sqrt() / b.norm().double().clamp_min(1e-12)).item()
        worst = max(worst, e)
        assert e <= 1e-5, (k, e)
        assert top.max().item() <= 12 * 4e-4, (k, top.max().item())
        flipped += int((top > 1e-4).sum())
    for k in ("errD", "errG", "errD_real", "errD_fake"):
        a, b = float(res[1][0][k]), float(res[0][0][k])
        assert abs(a - b) <= (2e-4 if flipped else 1e-5) * abs(b) + 1e-6, (k, a, b)
    print(f"\n[entry point with --diffaug, {case}] graph replay vs eager launches after 6 iterations: worst parameter tensor {worst:.1e}"
          f" ({flipped} elements stepped the other way)")
    if case == "headline losses":
        plain, _ = _main(tmp_path, yml, "plain", "--graph", "0")
        assert float(plain["errD_fake"]) != float(res[0][0]["errD_fake"])


def test_off_by_default_no_diffaug_entry_point_is_called(tmp_path, monkeypatch):
    import xmc_gan.train_gan as tg
    cnt = _Count(monkeypatch)
    tg.main(["--cfg", _mini_yml(tmp_path), "--synthetic", "3", "--max_epoch", "1", "--precision", "fp32", "--seed", "11",
             "--output_dir", str(tmp_path / "run")])
    assert sum(cnt.n.values()) > 100 and cnt.diffaug() == {}
