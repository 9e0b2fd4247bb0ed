"""Micro-benchmark of CLIPScore's device side (not a test), with random weights at CLIP ViT-B/32's size (12 layers per tower; vision 768
wide, 12 heads, 224 px in 32 px patches; text 512 wide, 8 heads; projection 512).  On the same card, next to each figure, what a user would
otherwise run, in plain torch f32:

  front   the image front end alone, 256 images of 256 px -> the patch rows [256 * 49, 3072]: `ops.clip_patch_rows` (Pillow's integer bicubic,
          crop, table, patch order: two launches) against F.interpolate(mode='bicubic', antialias=True) + normalise + the same reshape.  The
          baseline is a float bicubic and not bit-equal to Pillow; it is there for the time only.
  images  6 000 images of 256 px through `CLIPScorer.encode_images` (in its own batches of 256) against the same forward in torch device ops
          behind that float front end
  text    256 captions of 20 tokens through `CLIPScorer.encode_text_ids` against the same forward in torch device ops

One process; per row 3 warm-up calls, then the median of `--windows` windows of `--calls` calls between device events (images: one call per
window).  One JSON line per row.

  python tests/bench_clip.py                 the whole table
  python tests/bench_clip.py --only text     one row"""
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
import clip_ref as R  # noqa: E402
from xmc_gan_amd import ops  # noqa: E402
from xmc_gan_amd.clip import CLIPScorer  # noqa: E402


def torch_front(u8, size, mean, std):
    """uint8 [N,H,W,3] -> normalised f32 [N,3,size,size]: the float antialiased bicubic a torch user has"""
    x = u8.permute(0, 3, 1, 2).float()
    x = F.interpolate(x, size=(size, size), mode="bicubic", antialias=True).round().clamp(0, 255) / 255.0
    return (x - mean[None, :, None, None]) / std[None, :, None, None]


def torch_layers(w, root, c, x, causal):
    B, T, H = x.shape
    heads, eps = c["num_attention_heads"], c["layer_norm_eps"]
    for i in range(c["num_hidden_layers"]):
        l = f"{root}encoder.layers.{i}."
        h = F.layer_norm(x, (H,), w[l + "layer_norm1.weight"], w[l + "layer_norm1.bias"], eps)
        qkv = F.linear(h, w[l + "qkv.weight"], w[l + "qkv.bias"]).view(B, T, 3, heads, H // heads).permute(2, 0, 3, 1, 4)
        ctx = F.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2], is_causal=causal).transpose(1, 2).reshape(B, T, H)
        x = x + F.linear(ctx, w[l + "self_attn.out_proj.weight"], w[l + "self_attn.out_proj.bias"])
        h = F.layer_norm(x, (H,), w[l + "layer_norm2.weight"], w[l + "layer_norm2.bias"], eps)
        up = F.linear(h, w[l + "mlp.fc1.weight"], w[l + "mlp.fc1.bias"])
        x = x + F.linear(up * torch.sigmoid(1.702 * up), w[l + "mlp.fc2.weight"], w[l + "mlp.fc2.bias"])
    return x


def torch_images(w, hf, u8, mean, std, batch=256):
    c = hf["vision_config"]
    H, P, eps = c["hidden_size"], c["patch_size"], c["layer_norm_eps"]
    v, outs = "vision_model.", []
    for lo in range(0, u8.shape[0], batch):
        px = torch_front(u8[lo:lo + batch], c["image_size"], mean, std)
        x = F.conv2d(px, w[v + "embeddings.patch_embedding.weight"], stride=P).flatten(2).transpose(1, 2)
        x = torch.cat([w[v + "embeddings.class_embedding"].expand(x.shape[0], 1, -1), x], 1) + w[v + "embeddings.position_embedding.weight"]
        x = F.layer_norm(x, (H,), w[v + "pre_layrnorm.weight"], w[v + "pre_layrnorm.bias"], eps)
        x = torch_layers(w, v, c, x, causal=False)
        pooled = F.layer_norm(x[:, 0], (H,), w[v + "post_layernorm.weight"], w[v + "post_layernorm.bias"], eps)
        outs.append(F.linear(pooled, w["visual_projection.weight"]))
    return torch.cat(outs)


def torch_text(w, hf, ids, lens):
    c = hf["text_config"]
    H, t = c["hidden_size"], "text_model."
    x = F.embedding(ids, w[t + "embeddings.token_embedding.weight"]) + w[t + "embeddings.position_embedding.weight"][:ids.shape[1]]
    x = torch_layers(w, t, c, x, causal=True)
    x = F.layer_norm(x, (H,), w[t + "final_layer_norm.weight"], w[t + "final_layer_norm.bias"], c["layer_norm_eps"])
    return F.linear(x[torch.arange(ids.shape[0], device=ids.device), lens - 1], w["text_projection.weight"])


def timed(fn, windows, calls):
    for _ in range(3):
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["front", "images", "text"], default=None)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--images", type=int, default=6000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tests/bench_clip.py measures on the MI355X; there is no CPU figure")
    dev = torch.device("cuda", 0)
    hf = R.hf_config(width=768, layers=args.layers, heads=12, ffn=3072, image=224, patch=32, vocab=49408, max_pos=77, dim=512,
                     text=dict(width=512, heads=8, ffn=2048))
    with tempfile.TemporaryDirectory() as d:
        _, w = R.write_model_dir(d, 1, hf)
        sc = CLIPScorer(d, dev)
    w = {k: v.to(dev) for k, v in w.items()}
    for root, c in (("vision_model.", hf["vision_config"]), ("text_model.", hf["text_config"])):          # the torch path gets the same fused QKV
        for i in range(c["num_hidden_layers"]):
            a = f"{root}encoder.layers.{i}."
            w[a + "qkv.weight"] = torch.cat([w.pop(a + f"self_attn.{n}_proj.weight") for n in "qkv"])
            w[a + "qkv.bias"] = torch.cat([w.pop(a + f"self_attn.{n}_proj.bias") for n in "qkv"])
    mean, std = torch.tensor(sc.mean, device=dev), torch.tensor(sc.std, device=dev)
    g = torch.Generator().manual_seed(0)
    rows = []

    def report(row, hip, plain, diff):
        for name, (med, lo, hi) in (("hip", hip), ("torch", plain)):
            row.update({f"{name}_ms": med, f"{name}_ms_min": lo, f"{name}_ms_max": hi})
        row.update(torch_over_hip=round(plain[0] / hip[0], 3), **diff)
        rows.append(row)
        print(json.dumps(row), flush=True)

    with torch.no_grad():
        if args.only in (None, "front"):
            u8 = torch.randint(0, 256, (256, 256, 256, 3), dtype=torch.uint8, generator=g).to(dev)
            hip = lambda: ops.clip_patch_rows(u8, 224, 224, 32, sc.lut())      # noqa: E731
            plain = lambda: torch_front(u8, 224, mean, std).reshape(256, 3, 7, 32, 7, 32).permute(0, 2, 4, 1, 3, 5).reshape(256 * 49, 3072)      # noqa: E731
            a, b = hip(), plain()
            report(dict(row="front", images=256, px=256, out_bytes=a.numel() * 4), timed(hip, args.windows, args.calls),
                   timed(plain, args.windows, args.calls), dict(max_abs_diff=float((a - b).abs().max()), share_of_values_equal=float((a == b).float().mean())))
        if args.only in (None, "images"):
            u8 = torch.randint(0, 256, (args.images, 256, 256, 3), dtype=torch.uint8, generator=g).to(dev)
            hip, plain = (lambda: sc.encode_images(u8)), (lambda: torch_images(w, hf, u8, mean, std))
            a, b = hip(), plain()
            flop = args.images * 50 * args.layers * 2 * (4 * 768 * 768 + 2 * 768 * 3072)
            report(dict(row="images", images=args.images, px=256, layers=args.layers, layer_gemm_tflop=flop / 1e12), timed(hip, args.windows, 1),
                   timed(plain, args.windows, 1), dict(feature_max_abs_diff=float((a - b).abs().max()), feature_rms=float(b.pow(2).mean().sqrt())))
        if args.only in (None, "text"):
            lengths = torch.randint(8, 21, (256,), generator=g).tolist()
            ids, lens = R.random_ids(hf, lengths, 20, seed=1)
            ids, lens = ids.to(dev), lens.to(dev)
            hip, plain = (lambda: sc.encode_text_ids(ids, lens)), (lambda: torch_text(w, hf, ids, lens))
            a, b = hip(), plain()
            report(dict(row="text", captions=256, tokens=20, layers=args.layers), timed(hip, args.windows, args.calls),
                   timed(plain, args.windows, args.calls), dict(feature_max_abs_diff=float((a - b).abs().max()), feature_rms=float(b.pow(2).mean().sqrt())))
    return rows


if __name__ == "__main__":
    main()
