"""FID between two image sets, on the HIP kernels of ``xmc_gan_amd.fid``.

    python xmc_gan/fid.py A B --inception PATH [--batch 100] [--save_stats A.npz] [--gpu 0]

``A`` and ``B`` are each a directory of PNG / JPEG images or an ``.npz`` statistics file (``mu``, ``sigma``: the cache format of
pytorch_fid, so existing COCO statistics work).  ``--inception`` is the FID Inception state dict (``pt_inception-2015-12-05-*.pth``;
default: $XMC_FID_INCEPTION) and is needed only when a directory has to be scored.  ``--save_stats`` writes the statistics of ``A``.
Prints ``FID: x``.  INTEGRATION.md section 3.5 has the details.
"""
import os
import sys

PROJ_DIR = os.path.abspath(os.path.join(os.path.dirname(os.path.realpath(__file__)), os.pardir))
if PROJ_DIR not in sys.path:
    sys.path.append(PROJ_DIR)

import argparse


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='FID between two image directories / statistics files')
    parser.add_argument('a', metavar='A', help='image directory or .npz statistics')
    parser.add_argument('b', metavar='B', help='image directory or .npz statistics')
    parser.add_argument('--inception', type=str, default='', metavar='PATH',
                        help='FID Inception weights: the pt_inception-2015-12-05-*.pth state dict (default: $XMC_FID_INCEPTION)')
    parser.add_argument('--batch', type=int, default=100)
    parser.add_argument('--save_stats', type=str, default='', metavar='A.npz', help='write the statistics of A here')
    parser.add_argument('--gpu', dest='gpu_id', type=int, default=0)
    return parser.parse_args(argv)


def _check_args(args):
    """everything that can be refused before a device is touched; -> whether a directory has to be scored"""
    from xmc_gan_amd.evaluate import image_set_kind, resolve_weights
    from xmc_gan_amd.fid import list_images
    if args.batch < 1:
        raise SystemExit('--batch must be >= 1')
    need = False
    for p in (args.a, args.b):
        kind = image_set_kind(p)
        if kind is None:
            raise SystemExit(f'{p} is neither an image directory nor an .npz statistics file')
        if kind == 'dir':
            if len(list_images(p)) < 2:
                raise SystemExit(f'{p} holds fewer than two images (.png / .jpg / .jpeg): nothing to score')
            need = True
    if need:
        args.inception = resolve_weights(args.inception, 'XMC_FID_INCEPTION', '--inception')
    return need


def main(argv=None):
    args = parse_args(argv)
    need = _check_args(args)
    from xmc_gan_amd import fid as F
    extractor = None
    if need:
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError('xmc_gan/fid.py scores images on an MI355X (HIP kernels only); two .npz files need none')
        torch.cuda.set_device(args.gpu_id)
        try:
            extractor = F.InceptionFID(args.inception, torch.device('cuda', args.gpu_id))
        except (ImportError, ValueError) as e:
            raise SystemExit(str(e))
    try:
        sa, sb = F.stats_of(args.a, extractor, args.batch), F.stats_of(args.b, extractor, args.batch)
        value = F.frechet_distance(*sa, *sb)
    except ValueError as e:
        raise SystemExit(str(e))
    if args.save_stats:
        F.save_stats(args.save_stats, *sa)
    print(f'FID: {value}')
    return value


if __name__ == '__main__':
    main()
