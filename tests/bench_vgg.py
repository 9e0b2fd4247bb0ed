"""Micro-benchmark of the VGG term (TRAIN.ENCODER_LOSS.VGG; not a test), with random weights at VGG-19's size.  One JSON line per row.

  term    the VGG part of a generator step -- real forward without a graph, generated forward, generated backward to the image -- through
          `VGGContrast` in the current precision mode, beside the same network in plain torch (bf16, channels_last, F.conv2d / F.relu /
          F.max_pool2d) on the same card
  layers  which convolution kernel each of the 16 layers dispatches to, forward and data gradient, with its time and TFLOP/s (xmc_gan_amd.prof)
  stream  achieved GB/s of the four kernels of csrc/vgg.hip on the conv1_2 and conv2_2 maps, beside a device copy of 1 GB (the `copy` row of
          tests/diag/hbm_bw_probe.py)
  step    the training step through `train_gan.main(--synthetic)` with the term on or off (--vgg 1 / 0): ms per step and peak device memory;
          one process per setting, so that the peak is that setting's own

  python tests/bench_vgg.py --only term --px 256 --batch 256
  python tests/bench_vgg.py --only step --vgg 1 --px 256 --batch 256"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import vgg_ref as R  # noqa: E402
from xmc_gan_amd import lib as L  # noqa: E402
from xmc_gan_amd import ops, prof  # noqa: E402
from xmc_gan_amd.vgg import PLAN, VGG19Features, VGGContrast  # noqa: E402


def timed(fn, windows, calls):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    return round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)


def torch_features(x, weights):
    """[N,3,H,W] channels_last bf16 in [-1, 1] -> f32 rows [N,512]: what a torch user runs"""
    mean = torch.tensor(R.MEAN, device=x.device, dtype=x.dtype).view(1, 3, 1, 1)
    std = torch.tensor(R.STD, device=x.device, dtype=x.dtype).view(1, 3, 1, 1)
    h, layer = ((x + 1) / 2 - mean) / std, 0
    for v in PLAN:
        if v == "M":
            h = F.max_pool2d(h, 2)
        else:
            h = F.relu(F.conv2d(h, *weights[layer], padding=1))
            layer += 1
    return h.float().mean((2, 3))


def term_flop(batch, px):
    """MFMA FLOPs of the term: two forwards and one data-gradient pass over the 16 convolutions"""
    flop, cin, side = 0.0, 3, px
    for v in PLAN:
        if v == "M":
            side //= 2
        else:
            flop += 2.0 * batch * side * side * 9 * cin * v
            cin = v
    return 3 * flop


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["term", "layers", "stream", "step"], required=True)
    ap.add_argument("--px", type=int, default=256)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "f16", "fp32"])
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--torch", type=int, default=1, help="term: 0 leaves the plain-torch side out")
    ap.add_argument("--vgg", type=int, default=1, help="step: the term on (1) or off (0)")
    ap.add_argument("--steps", type=int, default=14)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tests/bench_vgg.py measures on the MI355X; there is no CPU figure")
    dev = torch.device("cuda", 0)
    ops.set_precision(args.precision)
    dt = ops.act_dtype()
    B, S = args.batch, args.px
    g = torch.Generator().manual_seed(0)
    weights = R.random_weights(0)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "vgg19.pth")
        R.write_weights_file(path, weights=weights)
        if args.only == "step":
            return step_row(args, path, d)
        net = VGG19Features(path, dev).warm()
    row = dict(row=args.only, px=S, batch=B, precision=args.precision)

    def images():
        return [((torch.rand(B, S, S, 8, generator=g) * 2 - 1).to(dt)).to(dev) for _ in range(2)]

    if args.only == "term":
        contrast = VGGContrast(net)
        real_h, fake_h = images()
        r = torch.randn(B, 512, generator=g).to(dev)

        def hip():
            fk = fake_h.detach().requires_grad_()
            _, rows = contrast.rows(real_h, fk)
            return torch.autograd.grad((rows * r).sum(), fk)[0]
        torch.cuda.reset_peak_memory_stats()
        med, lo, hi = timed(hip, args.windows, args.calls)
        row.update(hip_ms=med, hip_ms_min=lo, hip_ms_max=hi, tflop=round(term_flop(B, S) / 1e12, 2),
                   hip_tflops=round(term_flop(B, S) / med / 1e9, 1), hip_peak_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))
        if args.torch:
            wt = [(w.to(dev, torch.bfloat16).contiguous(memory_format=torch.channels_last), b.to(dev, torch.bfloat16)) for w, b in weights]
            nchw = lambda t: t[..., :3].permute(0, 3, 1, 2).to(torch.bfloat16)      # noqa: E731 -- (a channels_last view of the engine image)
            real_t, fake_t = nchw(real_h).contiguous(memory_format=torch.channels_last), nchw(fake_h).contiguous(memory_format=torch.channels_last)

            def plain():
                fk = fake_t.detach().requires_grad_()
                with torch.no_grad():
                    torch_features(real_t, wt)
                return torch.autograd.grad((torch_features(fk, wt) * r).sum(), fk)[0]
            med_t, lo_t, hi_t = timed(plain, args.windows, args.calls)
            row.update(torch_ms=med_t, torch_ms_min=lo_t, torch_ms_max=hi_t, torch_over_hip=round(med_t / med, 3))
        print(json.dumps(row), flush=True)
    elif args.only == "layers":
        _, fake_h = images()
        r = torch.randn(B, 512, generator=g).to(dev)
        for rep in range(3):                 # the third pass is the one recorded
            if rep == 2:
                prof.enable()
            fk = fake_h.detach().requires_grad_()
            torch.autograd.grad((net(fk) * r).sum(), fk)
            torch.cuda.synchronize()
        recs = prof.launches()
        prof.disable()
        for r_ in recs:
            print(json.dumps(dict(row="layers", px=S, batch=B, precision=args.precision, launch=r_.tag, kernel=r_.kernel, ms=round(r_.ms, 4),
                                  tflops=round(r_.flops / r_.ms / 1e9, 1), algorithmic_gbs=round(r_.nbytes / r_.ms / 1e6, 1))), flush=True)
    elif args.only == "stream":
        x1 = torch.empty(2 ** 29, dtype=torch.bfloat16, device=dev).zero_()
        y1 = torch.empty_like(x1)
        med, _, _ = timed(lambda: y1.copy_(x1), args.windows, 5)
        print(json.dumps(dict(row="stream", kernel="device copy, 1 GB bf16", ms=med, gbs=round(2 * x1.numel() * 2 / med / 1e6, 1))), flush=True)
        del x1, y1
        esz = 4 if dt == torch.float32 else 2
        img = images()[0]
        out = torch.empty_like(img)
        lib, p, st, code = L.load(), ops._p, ops._st, ops._code(dt)
        for name in ("xmc_vgg_prep_fwd", "xmc_vgg_prep_bwd"):
            fn = getattr(lib, name)
            med, _, _ = timed(lambda: L.check(fn(p(img), p(out), B, S, S, code, st()), name), args.windows, 5)
            print(json.dumps(dict(row="stream", kernel=name, map=f"{B}x{S}x{S}x8", precision=args.precision, ms=med,
                                  gbs=round(2 * img.numel() * esz / med / 1e6, 1))), flush=True)
        for what, side, C in (("conv1_2", S, 64), ("conv2_2", S // 2, 128)):
            z = torch.randn(B, side, side, C, generator=torch.Generator(device=dev).manual_seed(1), device=dev).to(dt)
            pz = torch.empty(B, side // 2, side // 2, C, dtype=dt, device=dev)
            dz = torch.empty_like(z)
            med, _, _ = timed(lambda: L.check(lib.xmc_relu_maxpool2_fwd(p(z), p(pz), B, side, side, C, code, st()), "fwd"), args.windows, 5)
            print(json.dumps(dict(row="stream", kernel="xmc_relu_maxpool2_fwd", map=f"{what} {B}x{side}x{side}x{C}", precision=args.precision, ms=med,
                                  gbs=round((z.numel() + pz.numel()) * esz / med / 1e6, 1))), flush=True)
            med, _, _ = timed(lambda: L.check(lib.xmc_relu_maxpool2_bwd(p(z), p(pz), p(dz), B, side, side, C, code, st()), "bwd"), args.windows, 5)
            print(json.dumps(dict(row="stream", kernel="xmc_relu_maxpool2_bwd", map=f"{what} {B}x{side}x{side}x{C}", precision=args.precision, ms=med,
                                  gbs=round((2 * z.numel() + pz.numel()) * esz / med / 1e6, 1))), flush=True)
            del z, pz, dz


def step_row(args, weights_path, tmp):
    """``--steps`` iterations of df_gan_damsm_nomagp.yml through the entry point, the term on or off"""
    import xmc_gan.train_gan as tg
    txt = open(os.path.join(ROOT, "xmc_gan", "cfg", "df_gan_damsm_nomagp.yml")).read()
    assert "VGG: false" in txt
    yml = os.path.join(tmp, "step.yml")
    with open(yml, "w") as f:
        f.write(txt.replace("VGG: false", "VGG: true") if args.vgg else txt)
    torch.cuda.reset_peak_memory_stats()
    last = tg.main(["--cfg", yml, "--synthetic", str(args.steps), "--bs", str(args.batch), "--imsize", str(args.px), "--max_epoch", "1",
                    "--precision", args.precision, "--output_dir", os.path.join(tmp, "run")] + (["--vgg_weights", weights_path] if args.vgg else []))
    thr = last.get("throughput") or {}
    row = dict(row="step", vgg=bool(args.vgg), px=args.px, batch=args.batch, precision=args.precision, ms_per_step=thr.get("ms_per_step"),
               timed_steps=thr.get("steps"), hipgraph=bool(last.get("hipgraph")), peak_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
               vgg_loss=float(last["vgg_loss"]) if "vgg_loss" in last else None, errG=float(last["errG"]))
    print(json.dumps(row), flush=True)
    return row


if __name__ == "__main__":
    main()
