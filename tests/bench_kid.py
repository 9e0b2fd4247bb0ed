"""Benchmark of KID and the Inception Score kernel (not a test): one JSON line per size.

  KID: `xmc_gan_amd.manifold.kid` at S = 100 subsets of m = 1000 rows, D = 2048, on banks of N real and N generated rows (the draw on the
  host and the copy of the index tables included; `kernel_ms` is `ops.poly_mmd_sums` alone, the tables already on the device: its check
  of the tables against the banks, a device min / max with one host synchronisation per table, is inside the window) -- beside
  the same sums from plain torch f32 on the same card: `index_select` of a chunk of subsets, batched `bmm`, `pow`, sums (the m x m
  matrices of a chunk exist there: 4 MB per subset and Gram).  Two rates: `kernel_TFLOPs` counts the tiles the kernel computes, 2 * 128^2 * D
  each, padding rows included (the within-set Grams' lower tiles are not computed): the kernel's own rate, beside the 155 TF/s f32-MFMA
  ceiling.  `useful_TFLOPs_equivalent` counts what the definition asks for, 3 Grams of 2 * m^2 * D per subset -- what torch's path
  computes -- over the same time; the symmetry shortcut can put it above the ceiling.
  IS: `ops.inception_score_sums` on N x 1008 logits against torch's f64 softmax formulation (`log_softmax` in f64, `exp`, sums per part).
  The two paths alternate, `--reps` windows each; every window's time is printed, and the peak memory a path allocates beyond its inputs.

  python tests/bench_kid.py                       N = 6 000 and 30 000
  python tests/bench_kid.py --n 6000 --reps 2     a short run to put under a kernel trace"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from bench_manifold import features, window  # noqa: E402
from xmc_gan_amd import fid as FID  # noqa: E402
from xmc_gan_amd import lib as L  # noqa: E402
from xmc_gan_amd import manifold as MF  # noqa: E402
from xmc_gan_amd import ops  # noqa: E402

MFMA_F32_TFLOPS = 155.0


def torch_sums(real, fake, ir, jf, chunk):
    """[S,3] f64: the three sums of every subset from gathered copies and batched matrix products, `chunk` subsets at a time"""
    d, m = real.shape[1], ir.shape[1]
    out = []
    for lo in range(0, ir.shape[0], chunk):
        x = real.index_select(0, ir[lo:lo + chunk].reshape(-1)).view(-1, m, d)
        y = fake.index_select(0, jf[lo:lo + chunk].reshape(-1)).view(-1, m, d)
        kxx, kyy, kxy = ((torch.bmm(a, b.transpose(1, 2)) / d + 1.0).pow(3) for a, b in ((x, x), (y, y), (x, y)))
        tr = lambda k: k.diagonal(dim1=1, dim2=2).double().sum(1)          # noqa: E731
        out.append(torch.stack([kxx.double().sum((1, 2)) - tr(kxx), kyy.double().sum((1, 2)) - tr(kyy), kxy.double().sum((1, 2))], 1))
    return torch.cat(out)


def torch_is(logits, splits):
    logp = torch.log_softmax(logits.double(), 1)
    p = logp.exp()
    n = logits.shape[0]
    H = torch.stack([(p[s * n // splits:(s + 1) * n // splits] * logp[s * n // splits:(s + 1) * n // splits]).sum() for s in range(splits)])
    P = torch.stack([p[s * n // splits:(s + 1) * n // splits].sum(0) for s in range(splits)])
    return H, P


def alternate(paths, reps):
    for fn in paths.values():                      # every shape of the timed windows once: code objects, library algorithm choice
        fn()
    times, peak, last = {p: [] for p in paths}, {p: 0 for p in paths}, {}
    for _ in range(reps):
        for p, fn in paths.items():
            s, extra, last[p] = window(fn)
            times[p].append(round(s * 1e3, 3))
            peak[p] = max(peak[p], extra)
    return times, peak, last


def bench(n, d, subsets, size, reps, chunk, dev):
    real, fake = features(n, d, 2, 0.0, dev), features(n, d, 3, 0.15, dev)
    ir, jf = (torch.from_numpy(t).to(dev) for t in MF.kid_subsets(n, n, subsets, size))
    m = ir.shape[1]
    paths = {"kid": lambda: MF.kid(real, fake, subsets, size), "kernel": lambda: ops.poly_mmd_sums(real, fake, ir, jf),
             "torch": lambda: torch_sums(real, fake, ir.long(), jf.long(), chunk)}
    times, peak, last = alternate(paths, reps)
    best = {p: min(t) for p, t in times.items()}
    tiles = getattr(L.load(), "xmc_poly_mmd_tiles")(m)
    row = dict(what="kid", n=n, d=d, subsets=subsets, subset_size=m, reps=reps, torch_chunk_subsets=chunk, kid_ms=times["kid"], kernel_ms=times["kernel"],
               torch_ms=times["torch"], kernel_peak_extra_MB=round(peak["kernel"] / 2 ** 20, 2), torch_peak_extra_MB=round(peak["torch"] / 2 ** 20, 1),
               torch_over_kernel_best_of_each=round(best["torch"] / best["kernel"], 3),
               kernel_TFLOPs=round(subsets * tiles * 2.0 * 128 * 128 * d / (best["kernel"] * 1e-3) / 1e12, 1), mfma_f32_ceiling_TFLOPs=MFMA_F32_TFLOPS,
               useful_TFLOPs_equivalent=round(subsets * 3 * 2.0 * m * m * d / (best["kernel"] * 1e-3) / 1e12, 1),
               torch_useful_TFLOPs=round(subsets * 3 * 2.0 * m * m * d / (best["torch"] * 1e-3) / 1e12, 1),
               sums_difference_between_the_two_paths=float(((last["kernel"] - last["torch"]).abs() / last["torch"]).max()), kid=last["kid"]["kid"],
               kid_std=last["kid"]["std"])
    return row


def bench_is(n, c, splits, reps, dev):
    logits = (3.0 * torch.randn(n, c, generator=torch.Generator().manual_seed(5))).to(dev)
    paths = {"kernel": lambda: ops.inception_score_sums(logits, splits), "torch": lambda: torch_is(logits, splits)}
    times, peak, last = alternate(paths, reps)
    best = {p: min(t) for p, t in times.items()}
    score = lambda hp: FID.is_from_sums(hp[0].cpu().numpy(), hp[1].cpu().numpy(), n, splits)[0]          # noqa: E731
    return dict(what="inception_score", n=n, classes=c, splits=splits, reps=reps, kernel_ms=times["kernel"], torch_ms=times["torch"],
                kernel_peak_extra_MB=round(peak["kernel"] / 2 ** 20, 2), torch_peak_extra_MB=round(peak["torch"] / 2 ** 20, 1),
                torch_over_kernel_best_of_each=round(best["torch"] / best["kernel"], 3),
                kernel_GBps_of_the_logits=round(n * c * 4 / (best["kernel"] * 1e-3) / 1e9, 1), score_kernel=score(last["kernel"]), score_torch=score(last["torch"]))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[6000, 30000])
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--subsets", type=int, default=100)
    ap.add_argument("--subset_size", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=10, help="subsets per torch.bmm call")
    ap.add_argument("--is_n", type=int, default=30000)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tests/bench_kid.py measures on the MI355X; there is no CPU figure")
    dev = torch.device("cuda", 0)
    with torch.no_grad():
        for n in args.n:
            print(json.dumps(bench(n, args.d, args.subsets, args.subset_size, args.reps, args.chunk, dev)), flush=True)
        print(json.dumps(bench_is(args.is_n, 1008, 10, args.reps, dev)), flush=True)


if __name__ == "__main__":
    main()
