"""Inception Score of an image directory, on the HIP kernels of ``xmc_gan_amd.fid.InceptionScore`` (csrc/kid.hip).

    python xmc_gan/inception_score.py IMAGES_DIR --inception PATH [--splits 10] [--batch 100] [--gpu 0]

``--inception`` is the FID Inception state dict (``pt_inception-2015-12-05-*.pth``; default: $XMC_FID_INCEPTION); its ``fc.weight``
[1008, 2048] gives the logits (all 1008 outputs, no bias, as the original code and torch-fidelity).  The images are taken in sorted order
of their file names and cut into ``--splits`` consecutive parts, without shuffling.  Prints ``IS: mean +- spread``.  INTEGRATION.md
section 3.10.
"""
import os
import sys

PROJ_DIR = os.path.abspath(os.path.join(os.path.dirname(os.path.realpath(__file__)), os.pardir))
if PROJ_DIR not in sys.path:
    sys.path.append(PROJ_DIR)

import argparse


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Inception Score of an image directory')
    parser.add_argument('images', metavar='IMAGES_DIR', help='directory of PNG / JPEG images')
    parser.add_argument('--inception', type=str, default='', metavar='PATH',
                        help='FID Inception weights: the pt_inception-2015-12-05-*.pth state dict (default: $XMC_FID_INCEPTION)')
    parser.add_argument('--splits', type=int, default=10)
    parser.add_argument('--batch', type=int, default=100)
    parser.add_argument('--gpu', dest='gpu_id', type=int, default=0)
    return parser.parse_args(argv)


def _check_args(args):
    """everything that can be refused before a device is touched"""
    from xmc_gan_amd.evaluate import resolve_weights
    from xmc_gan_amd.fid import list_images
    if args.batch < 1:
        raise SystemExit('--batch must be >= 1')
    if args.splits < 1:
        raise SystemExit(f'--splits: {args.splits}; at least one part expected')
    if not os.path.isdir(args.images):
        raise SystemExit(f'{args.images} is not an image directory')
    n = len(list_images(args.images))
    if n < args.splits:
        raise SystemExit(f'{args.images} holds {n} images (.png / .jpg / .jpeg), fewer than --splits = {args.splits}')
    args.inception = resolve_weights(args.inception, 'XMC_FID_INCEPTION', '--inception')


def main(argv=None):
    args = parse_args(argv)
    _check_args(args)
    import torch
    from xmc_gan_amd import fid as F
    if not torch.cuda.is_available():
        raise RuntimeError('xmc_gan/inception_score.py runs on an MI355X (HIP kernels only)')
    torch.cuda.set_device(args.gpu_id)
    device = torch.device('cuda', args.gpu_id)
    try:
        extractor = F.InceptionFID(args.inception, device)
        r = F.accumulate(F.InceptionScore(extractor, args.splits), _in_file_order(args.images, extractor, args.batch)).finalize()
    except (ImportError, ValueError) as e:
        raise SystemExit(str(e))
    print(f'IS: {r["inception_score"]} +- {r["std"]} (splits={r["splits"]}, n={r["n"]})')
    return r


def _in_file_order(directory, extractor, batch):
    """the feature rows of the directory's images, one batch at a time, in sorted order of the file names: the parts are consecutive rows,
    so a batch whose files differ in size (`decoded_batches` groups them by size) is put back into file order"""
    import torch
    from xmc_gan_amd import fid as F
    files = F.list_images(directory)
    for i in range(0, len(files), batch):
        chunk = files[i:i + batch]
        rows = [None] * len(chunk)
        for idx, u8 in F.decoded_batches(chunk, batch):
            for j, row in zip(idx, extractor(u8)):
                rows[j] = row
        yield torch.stack(rows)


if __name__ == '__main__':
    main()
