"""Benchmark of the FID evaluation (not a test): features + statistics of 6 000 images at 256 px in batches of 100 (what `eval()` scores),
on the native path (`xmc_gan_amd.fid.InceptionFID` + `FeatureStats`: uint8 in, f64 moments out) and, on the same card with the same random
weights and images, the restatement of tests/fid_ref.py as plain torch device ops in f32 (F.interpolate, F.conv2d, F.batch_norm, torch's
pools; moments by a f64 matmul).  One process; each path runs one warm-up batch, then all batches between two device events.  One JSON line.

  python tests/bench_fid.py                         the two figures
  python tests/bench_fid.py --only hip --images 300  a short run to put under a kernel trace"""
import argparse
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import fid_ref as R  # noqa: E402
from xmc_gan_amd import fid as FID  # noqa: E402


def timed(step, nbatches):
    step(0)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(nbatches):
        step(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["hip", "torch"], default=None)
    ap.add_argument("--images", type=int, default=6000)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--size", type=int, default=256)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tests/bench_fid.py measures on the MI355X; there is no CPU figure")
    dev = torch.device("cuda", 0)
    sd = R.random_state_dict(1)
    nb = -(-args.images // args.batch)
    g = torch.Generator().manual_seed(2)
    pool = [torch.randint(0, 256, (args.batch, args.size, args.size, 3), dtype=torch.uint8, generator=g).to(dev) for _ in range(4)]
    row = dict(images=nb * args.batch, batch=args.batch, size=args.size)
    with torch.no_grad():
        if args.only != "torch":
            with tempfile.TemporaryDirectory() as d:
                torch.save(sd, os.path.join(d, "w.pth"))
                ex = FID.InceptionFID(os.path.join(d, "w.pth"), dev)
            st = FID.FeatureStats(device=dev)
            row["hip_s"] = round(timed(lambda i: st.update(ex(pool[i % 4])), nb), 3)
            mu_h, sig_h = st.finalize()
        if args.only != "hip":
            ref = R.trunk_f32_on(sd, dev)
            acc = dict(n=0, s=torch.zeros(2048, dtype=torch.float64, device=dev), o=torch.zeros((2048, 2048), dtype=torch.float64, device=dev))

            def step(i):
                f = ref.trunk(ref.front_end(pool[i % 4], 299).float()).double()
                acc["s"] += f.sum(0)
                acc["o"] += f.T @ f
                acc["n"] += f.shape[0]

            row["torch_s"] = round(timed(step, nb), 3)
            n = acc["n"]
            mu_t = (acc["s"] / n).cpu().numpy()
            sig_t = ((acc["o"] - n * torch.outer(acc["s"] / n, acc["s"] / n)) / (n - 1)).cpu().numpy()
        if args.only is None:
            row["torch_over_hip"] = round(row["torch_s"] / row["hip_s"], 3)
            row["fid_between_the_two_paths"] = FID.frechet_distance(mu_h, sig_h, mu_t, sig_t)        # the same images: ~0
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
