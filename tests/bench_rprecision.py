"""Benchmark of the R-precision evaluation (not a test), two parts, one JSON line each.

  encoder    image codes of 6 000 images at 256 px in batches of 100 (what `eval()` encodes): `CNN_ENCODER.encode_u8` on the native path and,
             on the same card with the same random weights and images, the restatement of tests/damsm_ref.py as plain torch device ops in f32.
             Run tests/bench_fid.py in the same session for the figure to hold it against: the trunk is the same 94 convolutions.
  retrieval  `ops.rprecision` at N = M = 30 000, K = 100, D = 256 (COCO's evaluation set against itself) beside torch's gather + bmm on the
             card (which materialises the [N,K,D] gather: 3 GB in f32, so it runs in chunks of 3 000 images).

  python tests/bench_rprecision.py                              both parts
  python tests/bench_rprecision.py --only encoder --images 300  a short run to put under a kernel trace"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import damsm_ref as R  # noqa: E402
from bench_fid import timed  # noqa: E402
from xmc_gan.model.encoder import CNN_ENCODER  # noqa: E402
from xmc_gan_amd import ops  # noqa: E402


def bench_encoder(args, dev):
    sd = R.random_state_dict(1, 256)
    nb = -(-args.images // args.batch)
    g = torch.Generator().manual_seed(2)
    pool = [torch.randint(0, 256, (args.batch, args.size, args.size, 3), dtype=torch.uint8, generator=g).to(dev) for _ in range(4)]
    row = dict(part="encoder", images=nb * args.batch, batch=args.batch, size=args.size)
    enc = CNN_ENCODER(256)
    enc.load_state_dict(sd, strict=True)
    enc = enc.to(dev).eval()
    last = {}
    row["hip_s"] = round(timed(lambda i: last.__setitem__("hip", enc.encode_u8(pool[i % 4])[1]), nb), 3)
    ref = R.Reference(sd)
    ref.sd = {k: v.to(dev, torch.float32) for k, v in ref.sd.items()}

    def step(i):
        x = 2.0 * (pool[i % 4].permute(0, 3, 1, 2).float() / 255.0) - 1.0
        last["torch"] = _forward_f32(ref, x, 299)[1]

    row["torch_s"] = round(timed(step, nb), 3)
    row["torch_over_hip"] = round(row["torch_s"] / row["hip_s"], 3)
    a, b = last["hip"].double(), last["torch"].double()
    row["code_difference_between_the_two_paths"] = float((a - b).abs().max() / b.pow(2).mean().sqrt())
    return row


def _forward_f32(self, x, resize_to=299):
    """`damsm_ref.Reference.forward` without its conversion to f64: the same calls on the f32 weights"""
    import torch.nn.functional as F
    with torch.no_grad():
        if resize_to is not None:
            x = F.interpolate(x, size=(resize_to, resize_to), mode="bilinear", align_corners=False)
        for n in ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"):
            x = self.conv(n, x)
        x = F.max_pool2d(x, 3, stride=2)
        x = self.conv("Conv2d_4a_3x3", self.conv("Conv2d_3b_1x1", x))
        x = F.max_pool2d(x, 3, stride=2)
        for m in ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            x = self.block(m, x)
        features = x
        for m in ("Mixed_7a", "Mixed_7b", "Mixed_7c"):
            x = self.block(m, x)
        code = F.linear(F.avg_pool2d(x, kernel_size=8).flatten(1), self.sd["emb_cnn_code.weight"], self.sd["emb_cnn_code.bias"])
        return F.conv2d(features, self.sd["emb_features.weight"]), code


def bench_retrieval(args, dev):
    N = M = args.n
    K, D = args.k, args.d
    g = torch.Generator().manual_seed(3)
    img, txt = torch.randn(N, D, generator=g).to(dev), torch.randn(M, D, generator=g).to(dev)
    rng = np.random.default_rng(0)
    cand = rng.integers(0, M, size=(N, K), dtype=np.int32)
    cand[:, 0] = np.arange(N)
    cand_d = torch.from_numpy(cand).to(dev)
    row = dict(part="retrieval", n=N, m=M, k=K, d=D, reps=args.reps)
    out = {}
    row["hip_ms"] = round(timed(lambda i: out.__setitem__("hip", ops.rprecision(img, txt, cand_d)), args.reps) / args.reps * 1e3, 3)
    chunk = 3000

    def step(i):
        ranks = []
        for lo in range(0, N, chunk):
            rows = txt[cand_d[lo:lo + chunk].long()]                                          # [chunk,K,D]: the gather
            dot = torch.bmm(rows, img[lo:lo + chunk, :, None]).squeeze(2)
            s = dot / (img[lo:lo + chunk].norm(dim=1)[:, None] * rows.norm(dim=2)).clamp(min=1e-8)
            ranks.append((s[:, 1:] > s[:, :1]).sum(1))
        out["torch"] = torch.cat(ranks)

    row["torch_ms"] = round(timed(step, args.reps) / args.reps * 1e3, 3)
    row["torch_over_hip"] = round(row["torch_ms"] / row["hip_ms"], 3)
    row["rows_that_differ"] = int((out["hip"].long() != out["torch"]).sum())                 # (ties within f32 rounding of each other only)
    # the traffic the kernel cannot avoid: every candidate row once (from L2 / MALL for the most part: txt is 31 MB)
    row["hip_gather_GB_per_s"] = round(N * K * D * 4 / (row["hip_ms"] * 1e-3) / 1e9, 1)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["encoder", "retrieval"], default=None)
    ap.add_argument("--images", type=int, default=6000)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--n", type=int, default=30000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tests/bench_rprecision.py measures on the MI355X; there is no CPU figure")
    dev = torch.device("cuda", 0)
    with torch.no_grad():
        if args.only != "retrieval":
            print(json.dumps(bench_encoder(args, dev)), flush=True)
        if args.only != "encoder":
            print(json.dumps(bench_retrieval(args, dev)), flush=True)


if __name__ == "__main__":
    main()
