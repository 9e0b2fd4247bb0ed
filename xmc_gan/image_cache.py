"""Build the uint8 image cache that ``train_gan.py --image_cache DIR`` trains from (xmc_gan_amd/imagecache.py: the format and the loader).

  python xmc_gan/image_cache.py build --data_dir data/coco --imsize 256 --split train [--out DIR] [--threads N]

Host only: decodes ``<data_dir>/images/<key>.jpg`` for every key of ``<data_dir>/<split>/filenames.pickle``, applies the split's Resize of
xmc_gan/dataset.py and writes ``<DIR>/<split>_<S>.u8`` and ``<DIR>/<split>_<S>.idx.npz`` (DIR defaults to ``<data_dir>/image_cache``).
Training needs both splits: run it once with ``--split train`` and once with ``--split test``.
"""
import argparse
import os
import sys
import time

PROJ_DIR = os.path.abspath(os.path.join(os.path.dirname(os.path.realpath(__file__)), os.pardir))
if PROJ_DIR not in sys.path:
    sys.path.append(PROJ_DIR)


def main(argv=None):
    ap = argparse.ArgumentParser(description="uint8 image cache for train_gan.py --image_cache")
    sub = ap.add_subparsers(dest="cmd", required=True)
    b = sub.add_parser("build", help="decode, resize and pack one split")
    b.add_argument("--data_dir", required=True)
    b.add_argument("--imsize", type=int, required=True)
    b.add_argument("--split", choices=["train", "test"], required=True)
    b.add_argument("--out", default="", help="cache directory (default: <data_dir>/image_cache)")
    b.add_argument("--threads", type=int, default=None, help="decoding threads, at most 16 (default: min(16, usable cores))")
    args = ap.parse_args(argv)
    from xmc_gan_amd.imagecache import build_cache
    t0 = time.perf_counter()
    u8, idx = build_cache(args.data_dir, args.imsize, args.split, args.out or None, args.threads)
    print(f"{u8}: {os.path.getsize(u8)} bytes, index {idx}, {time.perf_counter() - t0:.1f} s")
    return u8, idx


if __name__ == "__main__":
    main()
