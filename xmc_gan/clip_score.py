"""CLIPScore of a directory of generated images against their captions, on the HIP kernels of ``xmc_gan_amd.clip``.

    python xmc_gan/clip_score.py IMAGES_DIR --captions FILE --clip_dir PATH [--clip_max_tokens N] [--per_caption K] [--batch 100]
                                 [--gpu 0]

The PNG / JPEG files of ``IMAGES_DIR`` are taken in sorted order; caption ``i`` (line ``i`` of ``--captions``, blank lines skipped) belongs
to files ``i*K .. i*K+K-1`` (the order of ``sample.py``'s file names ``<caption:05d>_<k>.png``).  ``--clip_dir`` is a Hugging Face CLIPModel
directory, e.g. a copy of openai/clip-vit-base-patch32 (default: $XMC_CLIP_DIR); ``--clip_max_tokens 77`` or more scores at CLIP's own
text context and admits ViT-B/16 and ViT-L/14.  Prints the result as one JSON object: ``clip_score`` is
the mean of max(100 cos, 0) over the images (Hessel et al.'s 2.5 max(cos, 0) is 0.025 times it).  INTEGRATION.md section 3.11 has the details.
"""
import os
import sys

PROJ_DIR = os.path.abspath(os.path.join(os.path.dirname(os.path.realpath(__file__)), os.pardir))
if PROJ_DIR not in sys.path:
    sys.path.append(PROJ_DIR)

import argparse
import json


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='CLIPScore of generated images against their captions')
    parser.add_argument('images', metavar='IMAGES_DIR', help='directory of PNG / JPEG images, K consecutive files (sorted) per caption')
    parser.add_argument('--captions', type=str, required=True, metavar='FILE', help='one sentence per line')
    parser.add_argument('--clip_dir', type=str, default='', metavar='PATH', help='CLIPModel directory (default: $XMC_CLIP_DIR)')
    parser.add_argument('--clip_max_tokens', type=int, default=64, metavar='N',
                        help="the longest sequence CLIPScore's towers take (default 64: ViT-B/32 at a text context of 64, today's scores).  77 or more gives CLIP's own text context of 77 tokens and admits ViT-B/16 (197 tokens) and ViT-L/14 (257; 577 at 336 px); at most 1024")
    parser.add_argument('--per_caption', type=int, default=1, metavar='K')
    parser.add_argument('--batch', type=int, default=100)
    parser.add_argument('--gpu', dest='gpu_id', type=int, default=0)
    return parser.parse_args(argv)


def _check_args(args):
    """everything that can be refused before a device is touched; -> (the sorted image files, the sentences)"""
    from xmc_gan_amd.fid import list_images
    if args.per_caption < 1 or args.batch < 1:
        raise SystemExit('--per_caption and --batch must be >= 1')
    if not os.path.isdir(args.images):
        raise SystemExit(f'{args.images} is not a directory')
    files = list_images(args.images)
    if not files:
        raise SystemExit(f'{args.images} holds no image (.png / .jpg / .jpeg)')
    args.clip_dir = args.clip_dir or os.environ.get('XMC_CLIP_DIR', '')
    if not os.path.isfile(os.path.join(args.clip_dir, 'config.json')):
        raise SystemExit(f'a CLIP model directory is needed: --clip_dir PATH or XMC_CLIP_DIR (got {args.clip_dir!r})')
    if not os.path.isfile(args.captions):
        raise SystemExit(f'--captions: {args.captions} is not a file')
    with open(args.captions) as f:
        sents = [line.strip() for line in f if line.strip()]
    if len(files) != len(sents) * args.per_caption:
        raise SystemExit(f'{args.images} holds {len(files)} images, {len(sents)} captions x --per_caption {args.per_caption} = '
                         f'{len(sents) * args.per_caption} were expected')
    return files, sents


def main(argv=None):
    args = parse_args(argv)
    files, sents = _check_args(args)
    import torch
    from xmc_gan_amd.clip import CLIPScoreStats
    from xmc_gan_amd.evaluate import load_model
    from xmc_gan_amd.fid import decoded_batches
    if not torch.cuda.is_available():
        raise RuntimeError('xmc_gan/clip_score.py scores images on an MI355X (HIP kernels only)')
    torch.cuda.set_device(args.gpu_id)
    device = torch.device('cuda', args.gpu_id)
    try:
        stats = CLIPScoreStats(load_model('clip', args.clip_dir, device,
                                          **({} if args.clip_max_tokens == 64 else {'max_tokens': args.clip_max_tokens})))
    except (ImportError, ValueError, NotImplementedError) as e:
        raise SystemExit(f'--clip_dir: {e}')
    K = args.per_caption
    for idx, u8 in decoded_batches(files, args.batch):       # (the files of a batch that share a size go through the encoder together)
        mine = sorted({i // K for i in idx})
        stats.update(u8.to(device), [sents[c] for c in mine], [mine.index(i // K) for i in idx])
    result = stats.finalize()
    print(json.dumps(result))
    return result


if __name__ == '__main__':
    main()
