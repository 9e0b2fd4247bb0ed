"""Kernel Inception Distance between two image sets, on the HIP kernels of ``xmc_gan_amd.manifold.kid`` (csrc/kid.hip).

    python xmc_gan/kid.py REAL GENERATED --inception PATH [--subsets 100] [--subset_size 1000] [--seed 0] [--batch 100]
                          [--save_features REAL.npz] [--gpu 0]

Each side is a directory of PNG / JPEG images or an ``.npz`` feature file (``features`` [N,2048] f32 and ``n``, written by
``--save_features`` here or by xmc_gan/prdc.py).  A statistics file of FID (``mu``, ``sigma``) holds only moments and is refused.
``--inception`` is the FID Inception state dict (``pt_inception-2015-12-05-*.pth``; default: $XMC_FID_INCEPTION) and is needed only when a
directory has to be scored.  The polynomial kernel (x.y / D + 1)^3 and the unbiased MMD^2 over ``--subsets`` subsets of
min(``--subset_size``, rows of either side) rows, as torch-fidelity's defaults; the subsets are this project's own draw, so a value
differs from torch-fidelity's by sampling noise -- the printed spread.  Prints ``KID: mean +- spread``.  INTEGRATION.md section 3.10.
"""
import os
import sys

PROJ_DIR = os.path.abspath(os.path.join(os.path.dirname(os.path.realpath(__file__)), os.pardir))
if PROJ_DIR not in sys.path:
    sys.path.append(PROJ_DIR)

import argparse


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Kernel Inception Distance between two image directories / feature files')
    parser.add_argument('real', metavar='REAL', help='the real set: image directory or .npz feature file')
    parser.add_argument('generated', metavar='GENERATED', help='the generated set: image directory or .npz feature file')
    parser.add_argument('--inception', type=str, default='', metavar='PATH',
                        help='FID Inception weights: the pt_inception-2015-12-05-*.pth state dict (default: $XMC_FID_INCEPTION)')
    parser.add_argument('--subsets', type=int, default=100)
    parser.add_argument('--subset_size', type=int, default=1000)
    parser.add_argument('--seed', type=int, default=0)
    parser.add_argument('--batch', type=int, default=100)
    parser.add_argument('--save_features', type=str, default='', metavar='REAL.npz', help='write the feature rows of REAL here')
    parser.add_argument('--gpu', dest='gpu_id', type=int, default=0)
    return parser.parse_args(argv)


def _check_args(args):
    """everything that can be refused before a device is touched; -> whether a directory has to be scored"""
    from xmc_gan_amd.evaluate import image_set_kind, resolve_weights
    from xmc_gan_amd.fid import list_images
    from xmc_gan_amd.manifold import load_features
    if args.batch < 1:
        raise SystemExit('--batch must be >= 1')
    if args.subsets < 1:
        raise SystemExit(f'--subsets: {args.subsets}; at least one subset expected')
    if args.subset_size < 2:
        raise SystemExit(f'--subset_size: {args.subset_size}; at least two rows expected')
    need = False
    for p in (args.real, args.generated):
        kind = image_set_kind(p)
        if kind is None:
            raise SystemExit(f'{p} is neither an image directory nor an .npz feature file')
        if kind == 'dir':
            if len(list_images(p)) < 2:
                raise SystemExit(f'{p} holds fewer than two images (.png / .jpg / .jpeg): KID needs two rows per side')
            need = True
        else:
            try:
                rows = load_features(p).shape[0]
            except ValueError as e:
                raise SystemExit(str(e))
            if rows < 2:
                raise SystemExit(f'{p} holds {rows} rows: KID needs two rows per side')
    if need:
        args.inception = resolve_weights(args.inception, 'XMC_FID_INCEPTION', '--inception')
    return need


def main(argv=None):
    args = parse_args(argv)
    need = _check_args(args)
    import torch
    from xmc_gan_amd import manifold as MF
    if not torch.cuda.is_available():
        raise RuntimeError('xmc_gan/kid.py runs on an MI355X (HIP kernels only)')
    torch.cuda.set_device(args.gpu_id)
    device = torch.device('cuda', args.gpu_id)
    extractor = None
    if need:
        from xmc_gan_amd import fid as F
        try:
            extractor = F.InceptionFID(args.inception, device)
        except (ImportError, ValueError) as e:
            raise SystemExit(str(e))
    try:
        real, fake = MF.bank_of(args.real, extractor, args.batch, device), MF.bank_of(args.generated, extractor, args.batch, device)
        r = MF.kid(real, fake, args.subsets, args.subset_size, args.seed)
    except ValueError as e:
        raise SystemExit(str(e))
    if args.save_features:
        real.save(args.save_features)
    print(f'KID: {r["kid"]} +- {r["std"]} (subsets={r["subsets"]}, size={r["subset_size"]}, n={r["n_real"]}/{r["n_fake"]})')
    return r


if __name__ == '__main__':
    main()
