"""Micro-benchmark of `ops.attention_long` and of CLIPScore's image tower past 64 tokens (not a test).  On the same card, next to each
figure, what a user would otherwise run in plain torch f32:

  attention   warm, event-timed kernel time of `ops.attention_long` on a fused projection [B*T, 3H] against
              `torch.nn.functional.scaled_dot_product_attention` in f32 on the same tensors, and the achieved fraction of the 157 TF/s f32-MFMA
              peak by 4 T^2 64 FLOP per head (half of that for causal):
                b16   64 images x 12 heads x T = 197        l14   64 images x 16 heads x T = 257        text  256 captions x 8 heads x T = 77, causal
  short       `ops.attention_short` at T = 50 and 64 (64 images x 12 heads) beside `ops.attention_long` at the same T
  towers      `CLIPScorer.encode_images` of 512 images of 256 px through a full-depth random-weight ViT-B/16 (12 layers, 768 wide) and ViT-L/14
              (24 layers, 1024 wide) against the same forward in torch device ops (tests/bench_clip.py's)

One process; per row 3 warm-up calls, then the median of `--windows` windows of `--calls` calls between device events (towers: one call per
window).  One JSON line per row.

  python tests/bench_attention_long.py                    the whole table
  python tests/bench_attention_long.py --only attention   one part"""
import argparse
import json
import os
import sys
import tempfile

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import clip_ref as R  # noqa: E402
from bench_clip import timed, torch_images  # noqa: E402
from xmc_gan_amd import ops  # noqa: E402
from xmc_gan_amd.clip import CLIPScorer  # noqa: E402

PEAK_TFLOPS = 157.3          # f32 MFMA (= the f32 vector peak)


def sdpa(qkv, B, T, heads, causal):
    q, k, v = qkv.view(B, T, 3, heads, 64).permute(2, 0, 3, 1, 4)
    return F.scaled_dot_product_attention(q, k, v, is_causal=causal).transpose(1, 2).reshape(B * T, heads * 64)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["attention", "short", "towers"], default=None)
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tests/bench_attention_long.py measures on the MI355X; there is no CPU figure")
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    rows = []

    def report(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def ms(name, t):
        return {f"{name}_ms": t[0], f"{name}_ms_min": t[1], f"{name}_ms_max": t[2]}

    with torch.no_grad():
        if args.only in (None, "attention"):
            for name, B, heads, T, causal in (("b16", 64, 12, 197, False), ("l14", 64, 16, 257, False), ("text", 256, 8, 77, True)):
                qkv = torch.randn(B * T, 3 * heads * 64, generator=g).to(dev)
                hip, plain = (lambda: ops.attention_long(qkv, None, B, T, heads, causal=causal)), (lambda: sdpa(qkv, B, T, heads, causal))
                a, b = hip(), plain()
                th, tp = timed(hip, args.windows, args.calls), timed(plain, args.windows, args.calls)
                flop = B * heads * 4 * T * T * 64 * (0.5 if causal else 1.0)
                report(dict(row="attention", case=name, B=B, heads=heads, T=T, causal=causal, **ms("hip", th), **ms("torch_sdpa", tp),
                            torch_over_hip=round(tp[0] / th[0], 3), gflop=round(flop / 1e9, 3),
                            hip_tflops=round(flop / th[0] / 1e9, 2), share_of_f32_mfma_peak=round(flop / th[0] / 1e9 / PEAK_TFLOPS, 4),
                            max_abs_diff=float((a - b).abs().max())))
        if args.only in (None, "short"):
            B, heads = 64, 12
            for T in (50, 64):
                qkv = torch.randn(B * T, 3 * heads * 64, generator=g).to(dev)
                full = torch.full((B,), T, dtype=torch.int32, device=dev)
                short, long_ = (lambda: ops.attention_short(qkv, full, B, T, heads)), (lambda: ops.attention_long(qkv, None, B, T, heads))
                a, b = short(), long_()
                ts, tl = timed(short, args.windows, args.calls), timed(long_, args.windows, args.calls)
                report(dict(row="short", B=B, heads=heads, T=T, **ms("attention_short", ts), **ms("attention_long", tl),
                            short_over_long=round(ts[0] / tl[0], 3), max_abs_diff=float((a - b).abs().max())))
        if args.only in (None, "towers"):
            u8 = torch.randint(0, 256, (args.images, 256, 256, 3), dtype=torch.uint8, generator=g).to(dev)
            for name, width, layers, heads, patch, dim in (("ViT-B/16", 768, 12, 12, 16, 512), ("ViT-L/14", 1024, 24, 16, 14, 768)):
                hf = R.hf_config(width=width, layers=layers, heads=heads, ffn=4 * width, image=224, patch=patch, vocab=1000, max_pos=77, dim=dim,
                                 text=dict(width=512, heads=8, ffn=2048, layers=1))
                with tempfile.TemporaryDirectory() as d:
                    _, w = R.write_model_dir(d, 1, hf)
                    sc = CLIPScorer(d, dev, max_tokens=257)
                w = {k: v.to(dev) for k, v in w.items() if k.startswith("vis")}
                for i in range(layers):          # the torch path gets the same fused QKV
                    a = f"vision_model.encoder.layers.{i}."
                    w[a + "qkv.weight"] = torch.cat([w.pop(a + f"self_attn.{n}_proj.weight") for n in "qkv"])
                    w[a + "qkv.bias"] = torch.cat([w.pop(a + f"self_attn.{n}_proj.bias") for n in "qkv"])
                mean, std = torch.tensor(sc.mean, device=dev), torch.tensor(sc.std, device=dev)
                hip, plain = (lambda: sc.encode_images(u8)), (lambda: torch_images(w, hf, u8, mean, std))
                a, b = hip(), plain()
                th, tp = timed(hip, args.windows, 1), timed(plain, args.windows, 1)
                gemm = args.images * sc.tokens * layers * 2 * 12 * width * width
                att = args.images * heads * layers * 4 * sc.tokens ** 2 * 64
                report(dict(row="towers", model=name, images=args.images, tokens=sc.tokens, layers=layers, **ms("hip", th), **ms("torch", tp),
                            torch_over_hip=round(tp[0] / th[0], 3), layer_gemm_tflop=round(gemm / 1e12, 3), attention_tflop=round(att / 1e12, 3),
                            feature_max_abs_diff=float((a - b).abs().max()), feature_rms=float(b.pow(2).mean().sqrt())))
                del sc, w
                torch.cuda.empty_cache()
    return rows


if __name__ == "__main__":
    main()
