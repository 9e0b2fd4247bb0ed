"""Benchmark of the image-cache input path (not a test).  Generated images only.  Three measurements, one JSON line each:

  python tests/bench_imagecache.py kernel    (a) `ops.crop_flip_normalize` at S = 256, B = 256 over a pool of generated 304 x 405 images: time per
                                             launch between device events, achieved GB/s (bytes the algorithm needs: B * 3 * S * S source bytes
                                             read + 4 times as many written), and the same gather written in plain torch on the device
  python tests/bench_imagecache.py loader    (b) images/s of `DeviceImageLoader` alone (train=True, WORD captions), one epoch after a warm-up epoch,
                                             host clock around a loop that ends in a device synchronise
  python tests/bench_imagecache.py pil       (c) images/s of the PIL `DataLoader` path (8 workers) over a directory of generated 640 x 480 JPEGs;
                                             this process never opens the GPU

(a) and (b) need the MI355X; (c) must run in a process of its own."""
import argparse
import json
import os
import pickle
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _cfg(size):
    return types.SimpleNamespace(IMG=types.SimpleNamespace(SIZE=size), TEXT=types.SimpleNamespace(CAPTIONS_PER_IMAGE=5, MAX_LENGTH=20))


def _text_files(root, keys, rng):
    for mode in ("train", "test"):
        os.makedirs(os.path.join(root, mode), exist_ok=True)
        with open(os.path.join(root, mode, "filenames.pickle"), "wb") as f:
            pickle.dump(keys, f)
    caps = [list(rng.randint(1, 1000, size=rng.randint(5, 20))) for _ in range(len(keys) * 5)]
    i2w = {i: f"w{i}" for i in range(1000)}
    with open(os.path.join(root, "captions.pickle"), "wb") as f:
        pickle.dump([caps, caps, i2w, {v: k for k, v in i2w.items()}], f)


def _synthetic_cache(root, n, h, w, size, rng):
    """a cache in the tool's format without the decode: n generated h x w images (what Resize(304) makes of a 640 x 480 JPEG)"""
    from xmc_gan_amd import imagecache as IC
    keys = [f"k{i:06d}" for i in range(n)]
    _text_files(root, keys, rng)
    cache_dir = os.path.join(root, "cache")
    os.makedirs(cache_dir, exist_ok=True)
    u8, idx = IC.cache_paths(cache_dir, "train", size)
    stride = (h * w * 3 + 15) // 16 * 16
    distinct = rng.randint(0, 256, (min(n, 64), stride), dtype=np.uint8)          # 64 different images, repeated
    with open(u8, "wb") as f:
        for i in range(n):
            f.write(distinct[i % len(distinct)].tobytes())
        f.write(b"\0" * 16)
    with open(idx, "wb") as f:
        np.savez(f, offsets=np.arange(n, dtype=np.int64) * stride, heights=np.full(n, h, np.int32), widths=np.full(n, w, np.int32),
                 keys=np.array(keys, dtype=str), version=IC.FORMAT_VERSION, split="train", size=size, resize=IC.resize_rule("train", size)[1])
    return cache_dir, keys


def _events(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps          # ms per call


def bench_kernel(args):
    from xmc_gan import dataset as D
    from xmc_gan_amd import imagecache as IC, ops
    dev = torch.device("cuda", 0)
    S, B, h, w = args.size, args.batch, 304, 405
    rng = np.random.RandomState(0)
    with tempfile.TemporaryDirectory() as root:
        cache_dir, keys = _synthetic_cache(root, args.images, h, w, S, rng)
        ds = D.WordTextDataset(data_dir=root, mode="train", transform=None, cfg=_cfg(S))
        loader = IC.DeviceImageLoader(IC.ImageCache.load(cache_dir, "train", S, ds.filenames), ds, B, dev, train=True, reserve=0)
    idx = IC.epoch_indices(len(keys), B, 0, 1)
    params = IC.epoch_params(idx, loader.hw.host, S, 0, 1)
    rows = [ops.HostMirror(p, dev) for p in params[:8]]
    out = torch.empty((B, 3, S, S), dtype=torch.float32, device=dev)
    state = dict(i=0)

    def hip():
        ops.crop_flip_normalize(loader.pool, loader.offsets, loader.hw, rows[state["i"] % len(rows)], S, out=out, table=loader.table)
        state["i"] += 1

    # the same gather in plain torch: byte addresses [B,S,S,3] -> pool[addr] -> table -> NCHW
    ar = torch.arange(S, device=dev)

    def plain(p):
        off = loader.offsets[p[:, 0].long()]
        wd = loader.hw.dev[p[:, 0].long(), 1].long()
        y = (p[:, 1].long()[:, None] + ar[None, :])                                               # [B,S]
        x = torch.where(p[:, 3, None] != 0, S - 1 - ar[None, :], ar[None, :]) + p[:, 2].long()[:, None]      # [B,S]
        addr = off[:, None, None] + (y[:, :, None] * wd[:, None, None] + x[:, None, :]) * 3       # [B,S,S]
        addr = addr[:, None, :, :] + torch.arange(3, device=dev)[None, :, None, None]             # [B,3,S,S]
        return loader.table[loader.pool[addr].long()]

    ref = plain(rows[0].dev)
    state["i"] = 0
    hip()
    same = bool(torch.equal(out, ref))
    ms_hip = _events(hip, args.reps)
    ms_torch = _events(lambda: plain(rows[0].dev), max(3, args.reps // 10))
    nbytes = B * 3 * S * S * (1 + 4)
    print(json.dumps(dict(bench="kernel", size=S, batch=B, pool_images=len(keys), pool_bytes=int(loader.pool.numel()), image_hw=[h, w],
                          hip_ms=round(ms_hip, 4), hip_GBps=round(nbytes / ms_hip / 1e6, 1), torch_ms=round(ms_torch, 3),
                          torch_over_hip=round(ms_torch / ms_hip, 1), bit_equal_to_torch=same)), flush=True)


def bench_loader(args):
    from xmc_gan import dataset as D
    from xmc_gan_amd import imagecache as IC
    dev = torch.device("cuda", 0)
    S, B = args.size, args.batch
    rng = np.random.RandomState(0)
    with tempfile.TemporaryDirectory() as root:
        cache_dir, keys = _synthetic_cache(root, args.images, 304, 405, S, rng)
        ds = D.WordTextDataset(data_dir=root, mode="train", transform=None, cfg=_cfg(S))
        t0 = time.perf_counter()
        loader = IC.DeviceImageLoader(IC.ImageCache.load(cache_dir, "train", S, ds.filenames), ds, B, dev, train=True, reserve=0)
        torch.cuda.synchronize()
        t_up = time.perf_counter() - t0
    for _ in loader:                                    # warm-up epoch
        pass
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for _ in range(args.epochs):
        for imgs, texts, ks in loader:
            n += imgs.shape[0]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    step_rate = 256 / 42.9e-3                           # the G+D step: 256 images in 42.9 ms
    print(json.dumps(dict(bench="loader", size=S, batch=B, images=n, seconds=round(dt, 4), images_per_s=round(n / dt, 1),
                          ms_per_batch=round(1e3 * dt / (n / B), 4), step_images_per_s=round(step_rate, 1), over_step_rate=round(n / dt / step_rate, 2),
                          construct_and_upload_s=round(t_up, 3), pool_bytes=int(loader.pool.numel()))), flush=True)


def bench_pil(args):
    from PIL import Image
    from xmc_gan import dataset as D
    S, B = args.size, args.batch
    rng = np.random.RandomState(0)
    with tempfile.TemporaryDirectory() as root:
        os.makedirs(os.path.join(root, "images"))
        keys = [f"k{i:06d}" for i in range(args.jpegs)]
        small = rng.randint(0, 256, (60, 80, 3), dtype=np.uint8)
        for i, k in enumerate(keys):                    # photographic-like content: an upsampled random field, so the JPEG is of ordinary size
            a = np.roll(small, i, axis=1)
            Image.fromarray(a).resize((640, 480), Image.BICUBIC).save(os.path.join(root, "images", f"{k}.jpg"), quality=90)
        _text_files(root, keys, rng)
        ds = D.WordTextDataset(data_dir=root, mode="train", transform=D.train_transform(S), cfg=_cfg(S))
        loader = torch.utils.data.DataLoader(ds, batch_size=B, drop_last=True, shuffle=True, num_workers=args.workers, pin_memory=False,
                                             persistent_workers=args.workers > 0)
        for _ in loader:                                # warm-up epoch: workers started, files in the page cache
            pass
        t0 = time.perf_counter()
        n = 0
        for _ in range(args.epochs):
            for imgs, texts, ks in loader:
                n += imgs.shape[0]
        dt = time.perf_counter() - t0
        del loader
    assert not torch.cuda.is_initialized()
    print(json.dumps(dict(bench="pil", size=S, batch=B, workers=args.workers, jpegs=args.jpegs, images=n, seconds=round(dt, 3),
                          images_per_s=round(n / dt, 1), step_images_per_s=round(256 / 42.9e-3, 1))), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "loader", "pil"])
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--images", type=int, default=4096, help="images in the generated pool (304 x 405: 369 KB each)")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--jpegs", type=int, default=1024)
    ap.add_argument("--workers", type=int, default=8)
    args = ap.parse_args(argv)
    if args.what != "pil" and not torch.cuda.is_available():
        raise RuntimeError("tests/bench_imagecache.py kernel / loader measure on the MI355X; there is no CPU figure")
    dict(kernel=bench_kernel, loader=bench_loader, pil=bench_pil)[args.what](args)


if __name__ == "__main__":
    main()
