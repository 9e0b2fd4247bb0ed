"""Benchmark of precision / recall / density / coverage (not a test): one JSON line per size.

  What is timed: the two radius calls plus the two count calls of `xmc_gan_amd.manifold.prdc` (`ops.knn_radius2` x 2, `ops.manifold_count` x 2,
  the row norms included) on N real and N generated rows of D = 2048, k = 5 -- beside the same four results from plain torch on the same card:
  `torch.cdist` in row chunks (the N x N matrix would be 144 MB at 6 000 rows and 3.6 GB at 30 000), squared, `kthvalue` for the radii,
  compare-and-sum for the counts, `min` for the nearest distance.  The two paths alternate, `--reps` windows each; every window's time is
  printed, and the peak memory each path allocates beyond the inputs.  The rows are non-negative and near a rank-16 cone, as pooled ReLU
  features are.

  python tests/bench_manifold.py                       N = 6 000 and 30 000
  python tests/bench_manifold.py --n 6000 --reps 2     a short run to put under a kernel trace"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from xmc_gan_amd import ops  # noqa: E402


def features(n, d, seed, shift, dev):
    g = torch.Generator().manual_seed(seed)
    basis = torch.randn(16, d, generator=torch.Generator().manual_seed(1))
    w = torch.randn(n, 16, generator=g) + shift
    return torch.relu(w @ basis / 4.0 + 0.02 * torch.randn(n, d, generator=g)).to(dev)


def hip_path(real, fake, k):
    rad_r, rad_g = ops.knn_radius2(real, k), ops.knn_radius2(fake, k)
    cnt_g, _ = ops.manifold_count(fake, real, rad_r)
    cnt_r, near_r = ops.manifold_count(real, fake, rad_g)
    return rad_r, rad_g, cnt_g, cnt_r, near_r


def torch_path(real, fake, k, chunk):
    def radius(x):
        out = []
        for lo in range(0, x.shape[0], chunk):
            d = torch.cdist(x[lo:lo + chunk], x).square_()
            i = torch.arange(d.shape[0], device=x.device)
            d[i, lo + i] = float("inf")                                    # the row itself, by index
            out.append(d.kthvalue(k, dim=1).values)
        return torch.cat(out)

    def count(a, b, rb2):
        cnt, near = [], []
        for lo in range(0, a.shape[0], chunk):
            d = torch.cdist(a[lo:lo + chunk], b).square_()
            cnt.append((d <= rb2[None, :]).sum(1))
            near.append(d.min(1).values)
        return torch.cat(cnt), torch.cat(near)
    rad_r, rad_g = radius(real), radius(fake)
    cnt_g, _ = count(fake, real, rad_r)
    cnt_r, near_r = count(real, fake, rad_g)
    return rad_r, rad_g, cnt_g, cnt_r, near_r


def window(fn):
    """(seconds, peak bytes allocated beyond what was held at the start) of one call, by device events around it"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3, torch.cuda.max_memory_allocated() - held, out


def bench(n, d, k, reps, chunk, dev):
    real, fake = features(n, d, 2, 0.0, dev), features(n, d, 3, 0.15, dev)
    paths = {"hip": lambda: hip_path(real, fake, k), "torch": lambda: torch_path(real, fake, k, chunk)}
    for fn in paths.values():                      # every shape of the timed windows once: code objects, library algorithm choice
        fn()
    times, peak, last = {p: [] for p in paths}, {p: 0 for p in paths}, {}
    for _ in range(reps):
        for p, fn in paths.items():                # alternating
            s, extra, last[p] = window(fn)
            times[p].append(round(s * 1e3, 2))
            peak[p] = max(peak[p], extra)
    row = dict(n=n, d=d, k=k, reps=reps, torch_chunk_rows=chunk, hip_ms=times["hip"], torch_ms=times["torch"],
               hip_peak_extra_MB=round(peak["hip"] / 2 ** 20, 1), torch_peak_extra_MB=round(peak["torch"] / 2 ** 20, 1))
    best = {p: min(t) for p, t in times.items()}
    row["torch_over_hip_best_of_each"] = round(best["torch"] / best["hip"], 3)
    # 2 N^2 D flops per distance matrix, four matrices: the matrix rate the HIP path reaches end to end (not a kernel's share of peak)
    row["hip_TFLOPs_end_to_end"] = round(4 * 2.0 * n * n * d / (best["hip"] * 1e-3) / 1e12, 1)
    h, t = last["hip"], last["torch"]
    rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().pow(2).mean().sqrt())          # noqa: E731
    row["radius_difference_between_the_two_paths"] = max(rel(h[0], t[0]), rel(h[1], t[1]))
    row["rows_whose_count_differs"] = int((h[2].long() != t[2]).sum()) + int((h[3].long() != t[3]).sum())
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[6000, 30000])
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=2000, help="rows per torch.cdist call")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tests/bench_manifold.py measures on the MI355X; there is no CPU figure")
    dev = torch.device("cuda", 0)
    with torch.no_grad():
        for n in args.n:
            print(json.dumps(bench(n, args.d, args.k, args.reps, args.chunk, dev)), flush=True)


if __name__ == "__main__":
    main()
