"""Micro-benchmark of the sentence encoder (not a test): the full 12-layer, 768-wide SBERT_ENCODER.forward_ids with random weights at
88 x 20 and 256 x 20 tokens in the fp32 and bf16 modes, and on the same card the same forward written with plain torch device ops (what a
user would otherwise run: every tensor in the mode's dtype, torch's own GEMMs and fused attention).  One process; per configuration 3 warm-up
calls, then the median of 7 windows of 10 calls between device events.  One JSON line per configuration.

  python tests/bench_sbert_encoder.py                       the whole table
  python tests/bench_sbert_encoder.py --only hip --modes bf16 --batches 256 --windows 1      a short run to put under a kernel trace"""
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
import sbert_ref as R  # noqa: E402
from xmc_gan.config import gan  # noqa: E402
from xmc_gan.model.encoder import SBERT_ENCODER  # noqa: E402
from xmc_gan_amd import ops  # noqa: E402


def torch_forward(w, hf, ids, lens, max_length, dtype):
    """the restatement of tests/sbert_ref.py as device ops in `dtype` (weights cast once by the caller)"""
    B, T = ids.shape
    H, heads, eps = hf["hidden_size"], hf["num_attention_heads"], hf["layer_norm_eps"]
    valid = torch.arange(T, device=ids.device)[None, :] < lens[:, None]
    pos = torch.cumsum(valid.long(), 1) * valid.long() + hf["pad_token_id"]
    e = "embeddings."
    x = F.embedding(ids, w[e + "word_embeddings.weight"]) + w[e + "token_type_embeddings.weight"][0] + F.embedding(pos, w[e + "position_embeddings.weight"])
    x = F.layer_norm(x, (H,), w[e + "LayerNorm.weight"], w[e + "LayerNorm.bias"], eps)
    amask = valid[:, None, None, :]
    for i in range(hf["num_hidden_layers"]):
        l = f"encoder.layer.{i}."
        qkv = F.linear(x, w[l + "qkv.weight"], w[l + "qkv.bias"]).view(B, T, 3, heads, H // heads).permute(2, 0, 3, 1, 4)
        ctx = F.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2], attn_mask=amask).transpose(1, 2).reshape(B, T, H)
        x = F.layer_norm(F.linear(ctx, w[l + "attention.output.dense.weight"], w[l + "attention.output.dense.bias"]) + x, (H,),
                         w[l + "attention.output.LayerNorm.weight"], w[l + "attention.output.LayerNorm.bias"], eps)
        up = F.gelu(F.linear(x, w[l + "intermediate.dense.weight"], w[l + "intermediate.dense.bias"]))
        x = F.layer_norm(F.linear(up, w[l + "output.dense.weight"], w[l + "output.dense.bias"]) + x, (H,),
                         w[l + "output.LayerNorm.weight"], w[l + "output.LayerNorm.bias"], eps)
    emb = x.float() * valid[:, :, None]
    sent = emb.sum(1) / valid.sum(1, keepdim=True)
    words = F.pad(emb.transpose(1, 2), (0, max_length - T))
    return words.contiguous(), sent, F.pad(~valid, (0, max_length - T), value=True)


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
    return statistics.median(ms), min(ms), max(ms)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["hip", "torch"], default=None)
    ap.add_argument("--modes", default="bf16,fp32")
    ap.add_argument("--batches", default="88,256")
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tests/bench_sbert_encoder.py measures on the MI355X; there is no CPU figure")
    dev = torch.device("cuda", 0)
    gan.reset_cfg()
    gan.cfg_from_file(os.path.join(ROOT, "xmc_gan", "cfg", "df_gan_sbert_seperate.yml"))
    cfg = gan.cfg
    T = cfg.TEXT.MAX_LENGTH
    hf = R.hf_config(hidden=768, layers=args.layers, heads=12, ffn=3072, vocab=8192, max_pos=514)
    with tempfile.TemporaryDirectory() as d:
        _, w = R.write_model_dir(d, 1, hf)
        enc = SBERT_ENCODER(cfg, model_dir=d).to(dev)
    for i in range(hf["num_hidden_layers"]):           # the torch path gets the same fused QKV projection
        a = f"encoder.layer.{i}.attention.self."
        w[f"encoder.layer.{i}.qkv.weight"] = torch.cat([w.pop(a + n + ".weight") for n in ("query", "key", "value")])
        w[f"encoder.layer.{i}.qkv.bias"] = torch.cat([w.pop(a + n + ".bias") for n in ("query", "key", "value")])
    flop_per_token = hf["num_hidden_layers"] * 2 * (4 * 768 * 768 + 2 * 768 * 3072)           # the four GEMMs of a layer
    for mode in args.modes.split(","):
        ops.set_precision(mode)
        dt = ops.act_dtype()
        wt = {k: v.to(dev, dt) for k, v in w.items()} if args.only != "hip" else None
        for B in (int(b) for b in args.batches.split(",")):
            g = torch.Generator().manual_seed(B)
            lengths = torch.randint(8, T + 1, (B,), generator=g).tolist()
            lengths[0] = T
            ids, lens = R.random_batch(hf, lengths, T, seed=B)
            ids, lens = ids.to(dev), lens.to(dev)
            row = dict(mode=mode, batch=B, tokens=B * T, valid_tokens=sum(lengths), layers=hf["num_hidden_layers"],
                       gemm_tflop=flop_per_token * B * T / 1e12)
            with torch.no_grad():
                if args.only != "torch":
                    med, lo, hi = timed(lambda: enc.forward_ids(ids, lens), args.windows, args.calls)
                    row.update(hip_ms=round(med, 4), hip_ms_min=round(lo, 4), hip_ms_max=round(hi, 4))
                if args.only != "hip":
                    med, lo, hi = timed(lambda: torch_forward(wt, hf, ids, lens, T, dt), args.windows, args.calls)
                    row.update(torch_ms=round(med, 4), torch_ms_min=round(lo, 4), torch_ms_max=round(hi, 4))
                if args.only is None:
                    row["torch_over_hip"] = round(row["torch_ms"] / row["hip_ms"], 3)
                    a, b = enc.forward_ids(ids, lens), torch_forward(wt, hf, ids, lens, T, dt)
                    row["sent_embs_max_abs_diff"] = float((a[1] - b[1]).abs().max())          # the two paths compute the same thing
            print(json.dumps(row), flush=True)
    ops.set_precision("bf16")


if __name__ == "__main__":
    main()
