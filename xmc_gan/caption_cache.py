"""Build the caption-embedding cache that ``train_gan.py --caption_cache DIR`` trains from (xmc_gan_amd/captioncache.py: the format and
`CachedTextEncoder`).

  python xmc_gan/caption_cache.py build --cfg xmc_gan/cfg/<preset>.yml --data_dir data/coco --split train [--out DIR] [--bs N]
                                        [--sbert_dir PATH] [--precision bf16|f16|fp32] [--gpu N]

Needs the MI355X and the encoder: constructs the split's text dataset without images and the preset's frozen text encoder as train_gan.py
does (SBERT: ``--sbert_dir`` / $XMC_SBERT_DIR; RNN: ``TEXT.ENCODER_DIR``), encodes the one caption per image the datasets hand out in
batches of ``--bs`` (default: the preset's TRAIN.BATCH_SIZE; use the batch size and the ``--precision`` of the training run) and writes
``<DIR>/<split>.cap.f32`` and ``<DIR>/<split>.cap.idx.npz`` (DIR defaults to ``<data_dir>/caption_cache``).  Training needs both splits: run
it once with ``--split train`` and once with ``--split test``.
"""
import argparse
import os
import sys
import time

PROJ_DIR = os.path.abspath(os.path.join(os.path.dirname(os.path.realpath(__file__)), os.pardir))
if PROJ_DIR not in sys.path:
    sys.path.append(PROJ_DIR)


def main(argv=None):
    ap = argparse.ArgumentParser(description="caption-embedding cache for train_gan.py --caption_cache")
    sub = ap.add_subparsers(dest="cmd", required=True)
    b = sub.add_parser("build", help="encode one split's captions once")
    b.add_argument("--cfg", required=True)
    b.add_argument("--data_dir", required=True)
    b.add_argument("--split", choices=["train", "test"], required=True)
    b.add_argument("--out", default="", help="cache directory (default: <data_dir>/caption_cache)")
    b.add_argument("--bs", type=int, default=-1, help="captions per launch of the encoder (default: TRAIN.BATCH_SIZE of the preset)")
    b.add_argument("--sbert_dir", default="", help="SBERT presets: the RoBERTa model directory (default: $XMC_SBERT_DIR)")
    b.add_argument("--precision", default=None, choices=["bf16", "f16", "fp32"])
    b.add_argument("--gpu", dest="gpu_id", type=int, default=0)
    args = ap.parse_args(argv)
    import torch
    from xmc_gan.config.gan import cfg, cfg_from_file
    from xmc_gan_amd import ops
    from xmc_gan_amd.captioncache import build_cache, construct_encoder
    if not torch.cuda.is_available():
        raise RuntimeError("xmc_gan/caption_cache.py runs the text encoder on an MI355X (HIP kernels only)")
    cfg_from_file(args.cfg)
    if args.precision:
        ops.set_precision(args.precision)
    device = torch.device("cuda", args.gpu_id)
    torch.cuda.set_device(device)
    t0 = time.perf_counter()
    try:
        encoder, source = construct_encoder(cfg, device, args.sbert_dir or None, PROJ_DIR)
    except (ImportError, OSError) as e:
        raise SystemExit(f"caption_cache.py: the text encoder could not be constructed: {e}")
    f32, idx = build_cache(cfg, args.data_dir, args.split, encoder, args.out or None, args.bs if args.bs > 0 else None, source)
    print(f"{f32}: {os.path.getsize(f32)} bytes, index {idx}, {ops.precision()} mode, {time.perf_counter() - t0:.1f} s")
    return f32, idx


if __name__ == "__main__":
    main()
