"""Precision, recall, density and coverage between two image sets, on the HIP kernels of ``xmc_gan_amd.manifold``.

    python xmc_gan/prdc.py A B --inception PATH [--k 5] [--batch 100] [--save_features A.npz] [--gpu 0]

``A`` is the real set and ``B`` the generated one; each is a directory of PNG / JPEG images or an ``.npz`` feature file (``features`` [N,2048]
f32 and ``n``, written by ``--save_features``).  A statistics file of FID (``mu``, ``sigma``) holds only moments and is refused.
``--inception`` is the FID Inception state dict (``pt_inception-2015-12-05-*.pth``; default: $XMC_FID_INCEPTION) and is needed only when a
directory has to be scored.  The features are FID's Inception pool3 rows, not the VGG-16 features of the published precision / recall
figures.  Prints ``precision: p recall: r density: d coverage: c``.  INTEGRATION.md section 3.9 has the details.
"""
import os
import sys

PROJ_DIR = os.path.abspath(os.path.join(os.path.dirname(os.path.realpath(__file__)), os.pardir))
if PROJ_DIR not in sys.path:
    sys.path.append(PROJ_DIR)

import argparse


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='precision / recall / density / coverage between two image directories / feature files')
    parser.add_argument('a', metavar='A', help='the real set: image directory or .npz feature file')
    parser.add_argument('b', metavar='B', help='the generated set: image directory or .npz feature file')
    parser.add_argument('--inception', type=str, default='', metavar='PATH',
                        help='FID Inception weights: the pt_inception-2015-12-05-*.pth state dict (default: $XMC_FID_INCEPTION)')
    parser.add_argument('--k', type=int, default=5, help='nearest neighbours (1..16)')
    parser.add_argument('--batch', type=int, default=100)
    parser.add_argument('--save_features', type=str, default='', metavar='A.npz', help='write the feature rows of A here')
    parser.add_argument('--gpu', dest='gpu_id', type=int, default=0)
    return parser.parse_args(argv)


def _check_args(args):
    """everything that can be refused before a device is touched; -> whether a directory has to be scored"""
    from xmc_gan_amd.evaluate import image_set_kind, resolve_weights
    from xmc_gan_amd.fid import list_images
    from xmc_gan_amd.manifold import load_features
    if args.batch < 1:
        raise SystemExit('--batch must be >= 1')
    if not 1 <= args.k <= 16:
        raise SystemExit(f'--k: {args.k}; 1 <= k <= 16 expected')
    need = False
    for p in (args.a, args.b):
        kind = image_set_kind(p)
        if kind is None:
            raise SystemExit(f'{p} is neither an image directory nor an .npz feature file')
        if kind == 'dir':
            if len(list_images(p)) < args.k + 1:
                raise SystemExit(f'{p} holds fewer than k + 1 = {args.k + 1} images (.png / .jpg / .jpeg): no k-th neighbour')
            need = True
        else:
            try:
                rows = load_features(p).shape[0]
            except ValueError as e:
                raise SystemExit(str(e))
            if rows < args.k + 1:
                raise SystemExit(f'{p} holds {rows} rows, fewer than k + 1 = {args.k + 1}: no k-th neighbour')
    if need:
        args.inception = resolve_weights(args.inception, 'XMC_FID_INCEPTION', '--inception')
    return need


def main(argv=None):
    args = parse_args(argv)
    need = _check_args(args)
    import torch
    from xmc_gan_amd import manifold as MF
    if not torch.cuda.is_available():
        raise RuntimeError('xmc_gan/prdc.py runs on an MI355X (HIP kernels only)')
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
        real, fake = MF.bank_of(args.a, extractor, args.batch, device), MF.bank_of(args.b, extractor, args.batch, device)
        r = MF.prdc(real, fake, args.k)
    except ValueError as e:
        raise SystemExit(str(e))
    if args.save_features:
        real.save(args.save_features)
    print(f'precision: {r["precision"]} recall: {r["recall"]} density: {r["density"]} coverage: {r["coverage"]} '
          f'(k={r["k"]}, n={r["n_real"]}/{r["n_fake"]})')
    return r


if __name__ == '__main__':
    main()
