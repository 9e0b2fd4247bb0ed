"""The generator weight average (EMA) on the device: kernels, optimizer, iteration / graph replay, entry point, checkpoints.

The arithmetic bar is derived, not measured.  Reference: the recurrence ``e += (1 - d) (p - e)`` in float64 over the f32 weights
the product itself produced (read back after every step), ``d = float64(float32(decay))``.  For decay >= 0.5, ``1 - float32(decay)``
is exact in f32 (Sterbenz), so the only error is the rounding of the update: at most 4 roundings of relative size 2^-24 on
quantities bounded by ``M = max(|e|, |p|)`` over the run, and the previous error is multiplied by d <= 1.  After K updates, per
tensor: ``max |e_f32 - e_f64| <= 4 K 2^-24 M``.  During the warm-up (fewer than ``start`` updates applied) and for weights that did
not move the bar is ``torch.equal``."""
import ctypes as C
import json
import os
import pickle
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import xmc_ref as X
from golden_util import CFG_DIR
from parity_util import DEV, build_product, setup_cfg
from xmc_gan_amd import lib as L
from xmc_gan_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1,), (5,), (64, 32, 3, 3), (4099,), (7, 3)]


@pytest.fixture(autouse=True)
def _restore_precision():
    yield
    ops.set_precision("bf16")


class _Bag(torch.nn.Module):
    def __init__(self, ps):
        super().__init__()
        self.ps = torch.nn.ParameterList(ps)


class Recurrence:
    """the f64 reference over read-back weights, and the bound that goes with it"""

    def __init__(self, tensors, decay, start):
        self.e = [t.detach().double().cpu().clone() for t in tensors]
        self.d, self.start, self.n, self.k = float(np.float32(decay)), start, 0, 0
        self.M = [float(e.abs().max()) for e in self.e]

    def step(self, tensors):
        ps = [t.detach().double().cpu() for t in tensors]
        if self.n < self.start:
            self.e = [p.clone() for p in ps]
        else:
            self.e = [e + (1.0 - self.d) * (p - e) for e, p in zip(self.e, ps)]
            self.k += 1
        self.n += 1
        self.M = [max(m, float(p.abs().max()), float(e.abs().max())) for m, p, e in zip(self.M, ps, self.e)]

    def check(self, shadows, weights, what, factor=1.0):
        """-> the largest fraction of the bound used.  In the warm-up: bit-equal to the weights."""
        assert self.k <= 8
        worst = 0.0
        for i, (s, e, m) in enumerate(zip(shadows, self.e, self.M)):
            if self.n <= self.start:
                assert torch.equal(s, weights[i]), (what, i, "warm-up is a copy")
                continue
            bound = factor * 4 * self.k * 2.0 ** -24 * m
            err = float((s.detach().double().cpu() - e).abs().max())
            print(f"  [{what}] tensor {i}: |e_f32 - e_f64| = {err:.3e}, bound {bound:.3e} (K = {self.k}, M = {m:.3g})")
            assert err <= bound, (what, i, err, bound)
            worst = max(worst, err / bound if bound else 0.0)
        return worst


def _carve(flat, offset):
    """SHAPES as consecutive views of one flat buffer, the first at element `offset` (misaligned bases, as the data-parallel bucket has)"""
    out = []
    for s in SHAPES:
        n = int(np.prod(s))
        out.append(flat[offset: offset + n].view(s))
        offset += n
    assert offset <= flat.numel()
    return out


def _launch_standalone(shadows, params, decay, start, nupd):
    """xmc_ema_step through the C ABI on caller-owned tensors (what a caller outside `ParamEMA` does)"""
    chunk = L.load().xmc_adam_chunk_elems()
    ents = (L.EmaEntry * len(params))()
    chunks = []
    for i, (e, p) in enumerate(zip(shadows, params)):
        ents[i].shadow, ents[i].param, ents[i].n = e.data_ptr(), p.data_ptr(), p.numel()
        chunks += [(i, c) for c in range((p.numel() + chunk - 1) // chunk)]
    tab = torch.frombuffer(bytearray(bytes(ents)), dtype=torch.uint8).to(DEV)
    ch = torch.tensor(chunks, dtype=torch.int32).to(DEV)
    L.call("xmc_ema_step", C.c_void_p(tab.data_ptr()), len(params), C.c_void_p(ch.data_ptr()), len(chunks), float(decay), int(start),
           C.c_void_p(nupd.data_ptr()), None, 1, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()


@pytest.mark.parametrize("start", [0, 3])
@pytest.mark.parametrize("decay", [0.9, 0.999])
@pytest.mark.parametrize("layout", ["separate tensors", "carved from a flat buffer at odd offsets"])
def test_standalone_kernel_against_the_f64_recurrence(layout, decay, start):
    from xmc_gan_amd.optim import ParamEMA
    g = torch.Generator().manual_seed(3)
    total = sum(int(np.prod(s)) for s in SHAPES)
    init = [torch.randn(s, generator=g) for s in SHAPES]
    if layout == "separate tensors":
        params = [torch.nn.Parameter(t.to(DEV)) for t in init]
        ema = ParamEMA(_Bag(params), decay, start)
        shadows, nupd = ema.shadow, ema.num_updates
        update = ema.update
    else:
        pflat, sflat = torch.zeros(total + 8, device=DEV), torch.zeros(total + 8, device=DEV)
        params, shadows = _carve(pflat, 1), _carve(sflat, 3)         # parameters and shadows misaligned differently
        assert any(p.data_ptr() % 16 for p in params) and any((p.data_ptr() % 16) != (s.data_ptr() % 16) for p, s in zip(params, shadows))
        for p, s, t in zip(params, shadows, init):
            p.copy_(t)
            s.copy_(t)
        nupd = torch.zeros(1, dtype=torch.int32, device=DEV)
        update = lambda: _launch_standalone(shadows, params, decay, start, nupd)
        guard = (pflat[:1].clone(), pflat[1 + total:].clone(), sflat[:3].clone(), sflat[3 + total:].clone())
    ref = Recurrence(params, decay, start)
    still = 4                                        # this tensor is never perturbed: its shadow stays bit-equal to it
    worst = 0.0
    for it in range(6):
        with torch.no_grad():
            for i, p in enumerate(params):
                if i != still:
                    p.add_((4e-4 * torch.sign(torch.randn(p.shape, generator=g))).to(DEV))
        update()
        ref.step(params)
        assert int(nupd.item()) == it + 1
        worst = max(worst, ref.check(shadows, params, f"{layout}, decay {decay}, start {start}, update {it + 1}"))
        assert torch.equal(shadows[still], params[still])
    if layout != "separate tensors":                 # nothing written outside the carved tensors
        now = (pflat[:1], pflat[1 + total:], sflat[:3], sflat[3 + total:])
        assert all(torch.equal(a, b) for a, b in zip(guard, now))
    print(f"\n[standalone EMA, {layout}, decay {decay}, start {start}] worst fraction of the bound used: {worst:.3f}")


ADAM_SHAPES = [(5,), (1,), (64, 32, 3, 3), (4099,), (7, 3)]      # test_adam_matches_oracle_update's


def _adam_grads(g, it):
    """the gradients of test_adam_matches_oracle_update: at step 2 tensor 1 has none and tensor 3 has zeros"""
    grads = [torch.randn(s, generator=g) for s in ADAM_SHAPES]
    if it == 2:
        grads[1] = None
        grads[3] = torch.zeros(ADAM_SHAPES[3])
    return grads


@pytest.mark.parametrize("start", [0, 2])
def test_fused_adam_ema_step_leaves_adam_bit_identical_and_averages_every_tensor(start):
    from xmc_gan_amd.optim import HipAdam, ParamEMA
    g = torch.Generator().manual_seed(1)
    init = [torch.randn(s, generator=g) for s in ADAM_SHAPES]
    runs = {}
    for name in ("fused", "plain"):
        ps = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
        runs[name] = dict(ps=ps, opt=HipAdam(ps, lr=4e-4, betas=(0.0, 0.9)), ema=ParamEMA(_Bag(ps), 0.9, start))
    sd_before = runs["fused"]["opt"].state_dict()
    ref = Recurrence(init, 0.9, start)
    worst = 0.0
    for it in range(4):
        grads = _adam_grads(g, it)
        for r in runs.values():
            for p, gr in zip(r["ps"], grads):
                p.grad = None if gr is None else gr.to(DEV)
        runs["fused"]["opt"].step(ema=runs["fused"]["ema"])
        runs["plain"]["opt"].step()
        runs["plain"]["ema"].update()                 # adam_kernel + the standalone launch
        torch.cuda.synchronize()
        # the EMA must not perturb Adam: weights, moments, counters bit-identical
        for i, (a, b) in enumerate(zip(runs["fused"]["ps"], runs["plain"]["ps"])):
            assert torch.equal(a, b), (it, i)
            sa, sb = runs["fused"]["opt"].state[a], runs["plain"]["opt"].state[b]
            assert set(sa) == set(sb) == {"step", "exp_avg", "exp_avg_sq"}
            for k in sa:
                assert torch.equal(sa[k], sb[k]), (it, i, k)
        ref.step(runs["fused"]["ps"])
        for name in runs:
            assert int(runs[name]["ema"].num_updates.item()) == it + 1
            worst = max(worst, ref.check(runs[name]["ema"].shadow, runs[name]["ps"], f"{name}, step {it + 1}"))
        # fused and standalone agree within twice the bound (each is within it)
        for i, (a, b) in enumerate(zip(runs["fused"]["ema"].shadow, runs["plain"]["ema"].shadow)):
            if ref.n <= start:
                assert torch.equal(a, b)
            else:
                assert float((a.double() - b.double()).abs().max()) <= 2 * 4 * ref.k * 2.0 ** -24 * ref.M[i], (it, i)
    opt = runs["fused"]["opt"]
    assert opt.state[runs["fused"]["ps"][1]]["step"].item() == 3 and opt.state[runs["fused"]["ps"][0]]["step"].item() == 4
    # an attached EMA leaves the optimizer's state dict layout alone (it interchanges with torch.optim.Adam's)
    sd = opt.state_dict()
    assert set(sd) == set(sd_before) == {"state", "param_groups"} and sd["param_groups"] == sd_before["param_groups"]
    assert all(set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in sd["state"].values())
    print(f"\n[fused Adam + EMA, start {start}] worst fraction of the bound used: {worst:.3f}")


def test_fused_kernel_on_a_misaligned_flat_bucket():
    """parameters, gradients, moments and shadows carved from flat buffers at DIFFERENT element offsets: the fused launch equals
    adam_kernel + the standalone launch on separately allocated tensors, bit for bit (Adam) and within the bound (shadow)"""
    from xmc_gan_amd.optim import HipAdam, ParamEMA
    g = torch.Generator().manual_seed(7)
    total = sum(int(np.prod(s)) for s in SHAPES)
    init = [torch.randn(s, generator=g) for s in SHAPES]
    pflat, gflat = torch.zeros(total + 8, device=DEV), torch.zeros(total + 8, device=DEV)
    ps_m = [torch.nn.Parameter(v) for v in _carve(pflat, 1)]
    gs_m = _carve(gflat, 2)
    ps_a = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    with torch.no_grad():
        for p, t in zip(ps_m, init):
            p.copy_(t)
    opt_m, opt_a = HipAdam(ps_m, lr=4e-4, betas=(0.0, 0.9)), HipAdam(ps_a, lr=4e-4, betas=(0.0, 0.9))
    ema_m, ema_a = ParamEMA(_Bag(ps_m), 0.9, 1), ParamEMA(_Bag(ps_a), 0.9, 1)
    ref = Recurrence(init, 0.9, 1)
    for it in range(4):
        grads = [torch.randn(s, generator=g) for s in SHAPES]
        for p, gm, pa, gr in zip(ps_m, gs_m, ps_a, grads):
            gm.copy_(gr)
            p.grad = gm
            pa.grad = gr.to(DEV)
        opt_m.step(ema=ema_m)
        opt_a.step()
        ema_a.update()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(ps_m, ps_a)):
            assert torch.equal(a, b), (it, i)
            for k in ("step", "exp_avg", "exp_avg_sq"):
                assert torch.equal(opt_m.state[a][k], opt_a.state[b][k]), (it, i, k)
        ref.step(ps_m)
        ref.check(ema_m.shadow, ps_m, f"misaligned bucket, step {it + 1}")
    assert float(pflat[0]) == 0.0 and float(pflat[1 + total:].abs().max()) == 0.0      # nothing written outside the tensors


@pytest.mark.parametrize("layout", ["two groups and a tensor without gradient", "one group"])
def test_skipped_step_moves_nothing_shadow_and_counter_included(layout):
    from xmc_gan_amd.optim import HipAdam, ParamEMA
    torch.manual_seed(0)
    two = layout != "one group"
    ps = [torch.nn.Parameter(torch.randn(n, device=DEV)) for n in (1000, 37, 4096 * 5 + 3, 11)]
    opt = HipAdam([dict(params=ps[:2]), dict(params=ps[2:], lr=3e-4)] if two else ps, lr=1e-3, betas=(0.0, 0.9))
    ema = ParamEMA(_Bag(ps), 0.9, 0)
    sc = ops.LossScaler(DEV, init=1024.0, interval=100)

    def grads(bad):
        scale = float(sc.sf[0])
        for i, p in enumerate(ps):
            p.grad = None if (i == 3 and two) else torch.randn_like(p) * scale      # tensor 3 has no gradient: the standalone launch
        if bad:
            ps[2].grad.view(-1)[5] = float("inf")

    def snap():
        torch.cuda.synchronize()
        out = [p.detach().clone() for p in ps] + [e.clone() for e in ema.shadow]
        for p in ps:
            out += [v.clone() for v in opt.state[p].values()] if opt.state[p] else []
        return out, int(ema.num_updates.item())

    grads(False)
    opt.step(scaler=sc, ema=ema)                     # a finite step first: states exist, shadows differ from the weights
    with torch.no_grad():
        ps[3].add_(1.0)                              # (moves the gradient-less tensor away from its shadow)
    before, n_before = snap()
    assert n_before == 1
    grads(True)
    opt.step(scaler=sc, ema=ema)
    after, n_after = snap()
    st = sc.stats()
    assert st["last_step_skipped"] and st["skipped_steps"] == 1 and st["scale"] == 512.0
    assert n_after == n_before
    assert len(before) == len(after) and all(torch.equal(a, b) for a, b in zip(before, after))
    grads(False)
    opt.step(scaler=sc, ema=ema)                     # the next finite step updates all of it
    after2, n2 = snap()
    assert n2 == n_before + 1 and not sc.stats()["last_step_skipped"]
    moved = [not torch.equal(a, b) for a, b in zip(after, after2)]
    assert all(moved[:3]) and moved[3] == (not two)  # weights with a gradient moved, the gradient-less one did not ...
    assert all(moved[4:8])                           # ... and every shadow did, that tensor's included


def test_graph_replay_crosses_the_warm_up_boundary_without_recapture():
    from xmc_gan_amd.optim import HipAdam, ParamEMA
    g = torch.Generator().manual_seed(5)
    init = [torch.randn(s, generator=g) for s in SHAPES]
    all_grads = [[torch.randn(s, generator=g).to(DEV) for s in SHAPES] for _ in range(7)]
    res = {}
    for mode in ("eager", "graph"):
        ps = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
        static = [torch.zeros(s, device=DEV) for s in SHAPES]
        for p, s in zip(ps, static):
            p.grad = s
        opt, ema = HipAdam(ps, lr=4e-4, betas=(0.0, 0.9)), ParamEMA(_Bag(ps), 0.9, 3)

        def load(gr):
            for s, t in zip(static, gr):
                s.copy_(t)
        load(all_grads[0])
        opt.step(ema=ema)                            # one eager step either way (builds the tables outside capture)
        graph = None
        if mode == "graph":
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                opt.step(ema=ema)
        trace = []
        for it in range(1, 7):                       # updates 2 .. 7: the counter passes start = 3 on the way
            load(all_grads[it])
            graph.replay() if graph is not None else opt.step(ema=ema)
            torch.cuda.synchronize()
            trace.append([p.detach().clone() for p in ps] + [e.clone() for e in ema.shadow])
        res[mode] = (trace, int(ema.num_updates.item()), [int(opt.state[p]["step"].item()) for p in ps])
    assert res["eager"][1] == res["graph"][1] == 7 and res["eager"][2] == res["graph"][2] == [7] * len(SHAPES)
    for it, (a, b) in enumerate(zip(res["eager"][0], res["graph"][0])):
        assert all(torch.equal(x, y) for x, y in zip(a, b)), it          # same kernels, same order, no atomics: bit for bit
    tr = res["graph"][0]
    n = len(SHAPES)
    assert all(torch.equal(tr[0][i], tr[0][n + i]) for i in range(n))            # update 2 (< start): a copy
    assert not any(torch.equal(tr[3][i], tr[3][n + i]) for i in range(n))        # update 5 (>= start): an average


# ----------------------------------------------------------------------------------------------------------- the iteration
def _iteration_setup(n_critic=1, decay=0.9, start=1):
    import xmc_gan.train_gan as tg
    from xmc_gan_amd.optim import ParamEMA
    ops.set_precision("fp32")
    cfg, h = setup_cfg("df_gan_damsm_nomagp.yml", **{"TRAIN.NCH": 8, "TRAIN.N_CRITIC": n_critic})
    PG, PD = X.synth_params(X.gen_shapes(h), 5), X.synth_params(X.netd_shapes(h), 6)
    netG, netD, optG, optD = build_product(h, PG, PD, 1e-3)
    ema = ParamEMA(netG, decay, start)
    batches = []
    for i in range(5):
        b = X.synth_batch(h, 4, seed=500 + i, words_len=cfg.TEXT.MAX_LENGTH)
        batches.append([b[k].to(DEV) for k in ("imgs", "sent_embs", "words_embs", "mask", "noise")])
    opts = tg.StepOptions(ema=ema)
    fn = lambda i_, s_, w_, m_, n_, st: tg.gan_iteration(netG, netD, optG, optD, i_, s_, w_, m_, n_, st, opts)
    return tg, cfg, h, netG, netD, optG, optD, ema, batches, fn


@pytest.mark.parametrize("mode,n_critic", [("eager", 1), ("graph", 1), ("graph", 2)])
def test_iteration_updates_the_shadow_once_per_generator_step(mode, n_critic):
    from xmc_gan_amd.graph import GraphedIteration
    tg, cfg, h, netG, netD, optG, optD, ema, batches, fn = _iteration_setup(n_critic)
    # the keys an iteration returns today, from an iteration without the average
    netG0, netD0, optG0, optD0 = build_product(h, X.synth_params(X.gen_shapes(h), 5), X.synth_params(X.netd_shapes(h), 6), 1e-3)
    st0 = {"i": n_critic - 1}
    keys_today = set(tg.gan_iteration(netG0, netD0, optG0, optD0, *batches[0], st0))
    params = [p for _, p in netG.named_parameters()]
    ref = Recurrence(params, ema.decay, ema.start)
    runner = GraphedIteration(fn, batches[0], n_critic=n_critic, warmup=2) if mode == "graph" else None
    st, g_steps, worst = {}, 0, 0.0
    for it, b in enumerate(batches):
        out = runner(*b) if runner is not None else fn(*b, st)
        torch.cuda.synchronize()
        if "errG" in out:
            g_steps += 1
            assert set(out) == keys_today
            ref.step(params)
        assert int(ema.num_updates.item()) == g_steps, (it, g_steps)
        if g_steps:
            worst = max(worst, ref.check(ema.shadow, params, f"{mode}, N_CRITIC {n_critic}, iteration {it + 1}"))
    assert g_steps == 5 // n_critic
    assert not all(torch.equal(e, p) for e, p in zip(ema.shadow, params))         # past the warm-up the average is not the iterate
    if runner is not None:
        assert len(runner.seqs) == min(2, n_critic)
        runner.close()
    print(f"\n[iteration, {mode}, N_CRITIC {n_critic}] {g_steps} shadow updates, worst fraction of the bound used: {worst:.3f}")


def test_copy_to_never_serves_stale_packed_weights():
    from xmc_gan_amd.graph import GraphedIteration
    tg, cfg, h, netG, netD, optG, optD, ema, batches, fn = _iteration_setup()
    cls = type(netG)
    gen_ema = cls(tg.cfg).to(DEV).eval()
    fixed = dict(noise=batches[0][4].clone(), sent_embs=batches[0][1].clone(), words_embs=batches[0][2].clone(), mask=batches[0][3].clone())

    def run(gen):
        with torch.no_grad():
            return gen(**fixed).float().clone()

    def fresh_output():
        fresh = cls(tg.cfg).to(DEV)
        fresh.load_state_dict(netG.state_dict())                      # (buffers, if the class has any)
        missing, unexpected = fresh.load_state_dict(ema.state_dict()["shadow"], strict=False)
        assert not unexpected and not [k for k in missing if k in dict(fresh.named_parameters())]
        return run(fresh.eval())

    # two forwards of one module on one input are bit-equal (no atomics in the generator's forward): shown on the raw netG first
    netG.eval()
    raw_a, raw_b = run(netG), run(netG)
    netG.train()
    assert torch.equal(raw_a, raw_b)
    runner = GraphedIteration(fn, batches[0], n_critic=1, warmup=2)
    outs = []
    for it, b in enumerate(batches):
        runner(*b)
        if it in (2, 4):
            torch.cuda.synchronize()
            o = run(ema.copy_to(gen_ema))
            assert torch.equal(o, fresh_output()), f"after iteration {it + 1}: gen_ema ran on stale packed weights"
            netG.eval()
            raw = run(netG)
            netG.train()
            assert not torch.equal(o, raw)
            outs.append(o)
    assert not torch.equal(outs[0], outs[1])
    runner.close()


# ----------------------------------------------------------------------------------------------------------- the entry point
def _mini_yml(tmp_path, **subst):
    """df_gan_damsm.yml shrunk for a test run (thin network, tiny vocabulary, no pretrained encoder file)."""
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


def _mini_coco(root, n_img=8):
    from PIL import Image
    rng = np.random.RandomState(1)
    (root / "images").mkdir(parents=True)
    keys = [f"k{i:03d}" for i in range(n_img)]
    for k in keys:
        Image.fromarray(rng.randint(0, 256, (90, 100, 3), dtype=np.uint8)).save(root / "images" / f"{k}.jpg")
    for mode in ("train", "test"):
        (root / mode).mkdir()
        with open(root / mode / "filenames.pickle", "wb") as f:
            pickle.dump(keys, f)
    caps = [list(rng.randint(1, 40, size=rng.randint(2, 12))) for _ in range(n_img * 5)]
    i2w = {i: f"w{i}" for i in range(40)}
    with open(root / "captions.pickle", "wb") as f:
        pickle.dump([caps, caps, i2w, {v: k for k, v in i2w.items()}], f)
    return str(root)


def test_entry_point_updates_the_shadow_inside_the_replayed_graph(tmp_path):
    import xmc_gan.train_gan as tg
    yml = _mini_yml(tmp_path)
    common = ["--cfg", yml, "--synthetic", "6", "--max_epoch", "1", "--precision", "fp32", "--seed", "11"]
    # warm-up longer than the run: the shadow is a copy of the weights after EVERY step, so equality at the end proves the update
    # is part of the replayed graph and ran at the last step
    last = tg.main(common + ["--ema_decay", "0.9", "--ema_start", "100", "--graph", "1", "--output_dir", str(tmp_path / "warm")])
    assert last.get("hipgraph") is True
    ema, (netG, _) = tg.main.last_ema, tg.main.last_models
    sd = ema.state_dict()
    assert sd["num_updates"] == 6 and sd["decay"] == 0.9 and sd["start"] == 100
    named = dict(netG.named_parameters())
    assert set(sd["shadow"]) == set(named)
    for k, e in sd["shadow"].items():
        assert torch.equal(e, named[k].detach()), k
    # off: no average, and main says so
    tg.main(common + ["--graph", "1", "--output_dir", str(tmp_path / "off")])
    assert tg.main.last_ema is None
    # averaging from step 2 on: graph replay and eager launches agree under the rule the weights are compared by
    # (test_entry_point_graph_replay_equals_eager_launches: 1e-5 per tensor without its 1-in-10 000 most different elements, those
    # within 12 x the larger learning rate -- an average of weights that agree to that rule agrees to it)
    res = {}
    for graph in (1, 0):
        tg.main(common + ["--ema_decay", "0.9", "--ema_start", "2", "--graph", str(graph), "--output_dir", str(tmp_path / f"run{graph}")])
        sd = tg.main.last_ema.state_dict()
        assert sd["num_updates"] == 6
        res[graph] = {k: v.float().cpu() for k, v in sd["shadow"].items()}
        raw = dict(tg.main.last_models[0].named_parameters())
        assert not all(torch.equal(v, raw[k].detach()) for k, v in sd["shadow"].items())
    worst = 0.0
    for k, a in res[1].items():
        b = res[0][k]
        d = (a - b).abs().flatten().double()
        top = d.topk(max(1, d.numel() // 10000)).values
        e = ((d.square().sum() - top.square().sum()).clamp_min(0).sqrt() / b.norm().double().clamp_min(1e-12)).item()
        worst = max(worst, e)
        assert e <= 1e-5, (k, e)
        assert top.max().item() <= 12 * 4e-4, (k, top.max().item())
    print(f"\n[entry point, EMA] graph replay vs eager launches after 6 iterations: worst shadow tensor {worst:.1e}")


def test_entry_point_in_the_ieee_half_mode_counts_applied_generator_steps_only(tmp_path):
    """the half mode's optimizer step runs under the dynamic loss scale (`xmc_optim_step` with the scale and the shadow table, inside the replayed graph): the
    average advances once per generator step the scaler did NOT skip"""
    import xmc_gan.train_gan as tg
    ops.reset_loss_scalers()
    last = tg.main(["--cfg", _mini_yml(tmp_path), "--synthetic", "5", "--max_epoch", "1", "--precision", "f16", "--seed", "11",
                    "--ema_decay", "0.9", "--ema_start", "100", "--output_dir", str(tmp_path / "run")])
    assert last.get("hipgraph") is True
    skipped = ops.loss_scaler_stats()["G"]["skipped_steps"]
    ema, netG = tg.main.last_ema, tg.main.last_models[0]
    assert int(ema.num_updates.item()) == 5 - skipped
    for e, p in zip(ema.shadow, ema.params):          # warm-up: a copy of the weights after the last applied step
        assert torch.equal(e, p.detach())
    print(f"\n[entry point, f16 + EMA] {skipped} generator steps skipped by the loss scaler, {int(ema.num_updates.item())} shadow updates")


def test_checkpoint_eval_and_resume_with_the_average(tmp_path, monkeypatch, caplog):
    import xmc_gan.train_gan as tg
    data, run = _mini_coco(tmp_path / "coco"), str(tmp_path / "run")
    seen = []
    real_eval = tg.eval

    def spy(*a, **k):
        gen = k["netG"]
        seen.append((k["state_epoch"], gen, {n: p.detach().clone() for n, p in gen.named_parameters()}))
        return real_eval(*a, **k)
    monkeypatch.setattr(tg, "eval", spy)
    yml = _mini_yml(tmp_path, **{"MAX_EPOCH: 121": "MAX_EPOCH: 52"})
    args = ["--data_dir", data, "--output_dir", run, "--precision", "fp32", "--seed", "3", "--ema_decay", "0.9"]
    tg.main(["--cfg", yml] + args)
    model = os.path.join(run, "model")
    assert sorted(os.listdir(model)) == ["ema_state.pth", "netD_051.pth", "netD_052.pth", "netG_051.pth", "netG_052.pth",
                                         "netG_ema_051.pth", "netG_ema_052.pth", "optimizerD.pth", "optimizerG.pth"]
    assert torch.load(os.path.join(model, "ema_state.pth"), map_location="cpu") == dict(num_updates=52 * 2, decay=0.9, start=0)
    netG, ema = tg.main.last_models[0], tg.main.last_ema
    # a plain state dict with netG's keys
    fresh = type(netG)(tg.cfg)
    saved = torch.load(os.path.join(model, "netG_ema_052.pth"), map_location="cpu")
    fresh.load_state_dict(saved, strict=True)
    assert list(saved) == list(netG.state_dict())
    # eval() was handed the averaged generator: at the last epoch its weights are the shadow's, not the raw iterate's
    assert [e for e, _, _ in seen] == [51, 52]
    _, gen, weights = seen[-1]
    assert gen is not netG and not gen.training and netG.training
    shadow, raw = ema.state_dict()["shadow"], dict(netG.named_parameters())
    assert all(torch.equal(weights[k], shadow[k]) for k in shadow)
    assert not all(torch.equal(weights[k], raw[k].detach()) for k in shadow)
    assert all(torch.equal(saved[k], shadow[k].cpu()) for k in shadow)
    # resume for one more epoch: the counter continues
    yml2 = _mini_yml(tmp_path, **{"MAX_EPOCH: 121": "MAX_EPOCH: 53"})
    tg.main(["--cfg", yml2] + args + ["--resume_epoch", "52"])
    assert torch.load(os.path.join(model, "ema_state.pth"), map_location="cpu")["num_updates"] == 52 * 2 + 2
    assert "netG_ema_053.pth" in os.listdir(model)
    # a checkpoint written without the average: the shadow starts from netG_052.pth
    for f in ("netG_ema_052.pth", "ema_state.pth"):
        os.remove(os.path.join(model, f))
    seen_loaded = {}
    real_train = tg.train

    def no_train(*a, **k):
        seen_loaded.update({n: e.clone() for n, e in zip(k["opts"].ema.names, k["opts"].ema.shadow)})
        seen_loaded["__n"] = int(k["opts"].ema.num_updates.item())
        return {}
    monkeypatch.setattr(tg, "train", no_train)
    caplog.set_level("INFO")
    caplog.clear()
    tg.main(["--cfg", yml2] + args + ["--resume_epoch", "52"])
    monkeypatch.setattr(tg, "train", real_train)
    g052 = torch.load(os.path.join(model, "netG_052.pth"), map_location=DEV)
    assert seen_loaded.pop("__n") == 0
    assert all(torch.equal(e, g052[n]) for n, e in seen_loaded.items())
    assert "the EMA starts from netG_052.pth" in caplog.text           # ... and the log says so


def test_without_the_flag_no_new_file_is_written(tmp_path):
    import xmc_gan.train_gan as tg
    data, run = _mini_coco(tmp_path / "coco"), str(tmp_path / "run")
    yml = _mini_yml(tmp_path, **{"MAX_EPOCH: 121": "MAX_EPOCH: 51"})
    tg.main(["--cfg", yml, "--data_dir", data, "--output_dir", run, "--precision", "fp32", "--seed", "3", "--resume_epoch", "0"])
    assert sorted(os.listdir(os.path.join(run, "model"))) == ["netD_051.pth", "netG_051.pth", "optimizerD.pth", "optimizerG.pth"]
    assert tg.main.last_ema is None


# ----------------------------------------------------------------------------------------------------------- two ranks
def test_two_ranks_keep_identical_shadows(tmp_path):
    """data parallel: nothing is communicated for the average -- the weights are identical on every rank after the all-reduce, so the
    shadows are.  Checked, not assumed: two gloo ranks on one card (child processes), three iterations on different shards."""
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    out = tmp_path / "ema_dp.json"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(XMC_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", XMC_DUMP_AFTER="240")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "ema_dp_rehearsal.py"), "--out", str(out)]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    rep = json.loads(out.read_text())
    assert rep["world"] == 2 and rep["num_updates"] == [3, 3]
    assert rep["shadows_equal"] is True and rep["weights_equal"] is True and rep["shadow_differs_from_weights"] is True
