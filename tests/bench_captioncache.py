"""Benchmark of the caption-embedding cache (not a test).  Generated values only.  Two measurements, one JSON line each:

  python tests/bench_captioncache.py kernel     `ops.caption_gather` at B = 256, E = 768, T = 20 over generated tables of COCO train2014's size
                                                (82 783 captions, lengths uniform in 8..20): time per launch between device events, achieved GB/s
                                                (bytes the algorithm needs: the valid token rows and the sentence rows read, B*E*T + B*E floats
                                                and B*T bytes written), and beside it the same result from plain torch: three `index_select`s on
                                                zero-padded [N,E,T], [N,E] and [N,T] tables; the resident bytes of both layouts
  python tests/bench_captioncache.py encoder    `SBERT_ENCODER.forward_ids` at 256 x 20 with random RoBERTa-base-sized weights next to
                                                `CachedTextEncoder.forward_keys` on the same captions (a cache written from that forward's outputs)

Per measurement 3 warm-up calls, then the median of 7 windows of `--calls` calls between device events; `forward_keys` also by the host clock
(it ends in no synchronisation: the figure is what the host spends per call).  Both need the MI355X."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


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


def bench_kernel(args):
    from xmc_gan_amd import ops
    dev = torch.device("cuda", 0)
    N, B, E, T = args.captions, args.batch, args.emb, args.length
    rng = np.random.default_rng(0)
    lens_h = rng.integers(8, T + 1, size=N).astype(np.int32)
    off_h = np.zeros(N, np.int64)
    off_h[1:] = np.cumsum(lens_h.astype(np.int64))[:-1]
    rows_tok = int(lens_h.sum())
    g = torch.Generator(device=dev).manual_seed(0)
    sent_tab = torch.randn(N, E, device=dev, generator=g)
    tok_tab = torch.randn(rows_tok, E, device=dev, generator=g)
    lens, off = torch.from_numpy(lens_h).to(dev), torch.from_numpy(off_h).to(dev)
    # the padded layout plain torch gathers from
    valid = torch.arange(T, device=dev)[None, :] < lens[:, None]
    padded = torch.zeros(N, T, E, device=dev)
    padded[valid] = tok_tab
    words_pad = padded.permute(0, 2, 1).contiguous()
    del padded
    mask_pad = ~valid
    batches = [ops.HostMirror(rng.permutation(N)[:B].astype(np.int32), dev) for _ in range(8)]
    longs = [b.dev.long() for b in batches]
    out = (torch.empty(B, E, T, device=dev), torch.empty(B, E, device=dev), torch.empty(B, T, dtype=torch.bool, device=dev))
    state = dict(i=0)

    def hip():
        ops.caption_gather(sent_tab, tok_tab, off, lens, batches[state["i"] % 8], T, out=out)
        state["i"] += 1

    def plain():
        r = longs[state["i"] % 8]
        state["i"] += 1
        return words_pad.index_select(0, r), sent_tab.index_select(0, r), mask_pad.index_select(0, r)

    state["i"] = 0
    hip()
    state["i"] = 0
    same = all(bool(torch.equal(a, b)) for a, b in zip(out, plain()))
    hip_ms = timed(hip, args.windows, args.calls)
    torch_ms = timed(plain, args.windows, args.calls)
    mean_valid = float(lens_h.mean())
    nbytes = B * E * 4 * (mean_valid + T + 2) + B * T
    print(json.dumps(dict(bench="kernel", captions=N, batch=B, emb=E, length=T, mean_valid_tokens=round(mean_valid, 2),
                          hip_ms=round(hip_ms[0], 4), hip_ms_min=round(hip_ms[1], 4), hip_ms_max=round(hip_ms[2], 4),
                          hip_GBps=round(nbytes / hip_ms[0] / 1e6, 1),
                          torch_ms=round(torch_ms[0], 4), torch_ms_min=round(torch_ms[1], 4), torch_ms_max=round(torch_ms[2], 4),
                          torch_over_hip=round(torch_ms[0] / hip_ms[0], 2), bit_equal_to_torch=same,
                          resident_bytes_valid_tokens=int((sent_tab.numel() + tok_tab.numel()) * 4 + N * 12),
                          resident_bytes_padded=int((sent_tab.numel() + words_pad.numel()) * 4 + mask_pad.numel()))), flush=True)


def bench_encoder(args):
    import sbert_ref as R
    from xmc_gan.config import gan
    from xmc_gan.model.encoder import SBERT_ENCODER
    from xmc_gan_amd import captioncache as CC, ops
    dev = torch.device("cuda", 0)
    gan.reset_cfg()
    gan.cfg_from_file(os.path.join(ROOT, "xmc_gan", "cfg", "df_gan_sbert_seperate.yml"))
    cfg = gan.cfg
    ops.set_precision(args.mode)
    B, T = args.batch, cfg.TEXT.MAX_LENGTH
    hf = R.hf_config(hidden=768, layers=12, heads=12, ffn=3072, vocab=8192, max_pos=514)
    with tempfile.TemporaryDirectory() as d:
        R.write_model_dir(d, 1, hf)
        enc = SBERT_ENCODER(cfg, model_dir=d).to(dev)
    g = torch.Generator().manual_seed(B)
    lengths = torch.randint(8, T + 1, (B,), generator=g).tolist()
    lengths[0] = T
    ids, lens = R.random_batch(hf, lengths, T, seed=B)
    ids_d, lens_d = ids.to(dev), lens.to(dev)
    words, sent, mask = enc.forward_ids(ids_d, lens_d)
    keys = [f"k{i:06d}" for i in range(B)]
    with tempfile.TemporaryDirectory() as d:
        w = CC.CacheWriter(d, "train", B, cfg.TEXT.EMBEDDING_DIM)
        w.add(sent.cpu().numpy(), words.transpose(1, 2)[~mask].cpu().numpy(), (~mask).sum(1).cpu().numpy())
        meta = dict(CC.cfg_meta(cfg), precision=args.mode, batch_size=B, captions_fingerprint="", encoder_fingerprint=CC.encoder_fingerprint(enc),
                    encoder_source="random weights")
        f32, _ = w.finish(keys, meta)
        cache = CC.CaptionCache(f32, w.lens, np.concatenate([[0], np.cumsum(w.lens.astype(np.int64))[:-1]]), keys, "train", meta)
        cached = CC.CachedTextEncoder(cache, dev, reserve=0)
    perm = [list(np.random.default_rng(i).permutation(B)) for i in range(8)]
    batches = [[keys[j] for j in p] for p in perm]
    got = cached.forward_keys(batches[0])
    p0 = torch.tensor(perm[0], device=dev)
    same = bool(torch.equal(got[0], words[p0]) and torch.equal(got[1], sent[p0]) and torch.equal(got[2], mask[p0]))
    state = dict(i=0)

    def from_cache():
        cached.forward_keys(batches[state["i"] % 8])
        state["i"] += 1

    with torch.no_grad():
        enc_ms = timed(lambda: enc.forward_ids(ids_d, lens_d), args.windows, max(1, args.calls // 5))
        cache_ms = timed(from_cache, args.windows, args.calls)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(200):
        from_cache()
    host_ms = (time.perf_counter() - t0) / 200 * 1e3
    torch.cuda.synchronize()
    print(json.dumps(dict(bench="encoder", mode=args.mode, batch=B, length=T, forward_ids_ms=round(enc_ms[0], 4), forward_ids_ms_min=round(enc_ms[1], 4),
                          forward_ids_ms_max=round(enc_ms[2], 4), forward_keys_ms=round(cache_ms[0], 4), forward_keys_ms_min=round(cache_ms[1], 4),
                          forward_keys_ms_max=round(cache_ms[2], 4), forward_keys_host_ms=round(host_ms, 4),
                          encoder_over_cache=round(enc_ms[0] / cache_ms[0], 1), bit_equal_to_the_encoder=same)), flush=True)
    ops.set_precision("bf16")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "encoder"])
    ap.add_argument("--captions", type=int, default=82783)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--emb", type=int, default=768)
    ap.add_argument("--length", type=int, default=20)
    ap.add_argument("--mode", default="bf16", choices=["bf16", "f16", "fp32"])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tests/bench_captioncache.py measures on the MI355X; there is no CPU figure")
    dict(kernel=bench_kernel, encoder=bench_encoder)[args.what](args)


if __name__ == "__main__":
    main()
