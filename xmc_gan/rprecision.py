"""R-precision of a directory of generated images against their captions, on the HIP kernels of ``xmc_gan_amd.rprecision``.

    python xmc_gan/rprecision.py IMAGES_DIR --cfg PRESET (--token_ids F.npy | --captions F) [--per_caption K]
                                 --image_encoder PATH --text_encoder PATH [--k 100 --splits 10 --seed 0] [--batch 100] [--gpu 0]

The PNG / JPEG files of ``IMAGES_DIR`` are taken in sorted order; caption ``i`` belongs to files ``i*K .. i*K+K-1`` (the order of
``sample.py``'s file names ``<caption:05d>_<k>.png``).  ``--image_encoder`` is the DAMSM image encoder (``image_encoder100.pth``; default:
$XMC_DAMSM_IMAGE_ENCODER); ``--text_encoder`` the caption encoder the preset names: the RNN state dict (``text_encoder100.pth``; default:
TEXT.ENCODER_DIR), or for an SBERT preset the RoBERTa model directory (default: $XMC_SBERT_DIR) -- whose sentence codes must have the image
encoder's width.  Prints the result as one JSON object.  INTEGRATION.md section 3.6 has the details.
"""
import os
import sys

PROJ_DIR = os.path.abspath(os.path.join(os.path.dirname(os.path.realpath(__file__)), os.pardir))
if PROJ_DIR not in sys.path:
    sys.path.append(PROJ_DIR)

import argparse
import json


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='R-precision of generated images against their captions')
    parser.add_argument('images', metavar='IMAGES_DIR', help='directory of PNG / JPEG images, K consecutive files (sorted) per caption')
    parser.add_argument('--cfg', type=str, required=True, help='the preset the images were sampled with')
    parser.add_argument('--token_ids', type=str, default='', metavar='FILE', help='.npy int64 [n, TEXT.MAX_LENGTH] token ids, 0-padded')
    parser.add_argument('--captions', type=str, default='', metavar='FILE', help='one sentence per line')
    parser.add_argument('--per_caption', type=int, default=1, metavar='K')
    parser.add_argument('--image_encoder', type=str, default='', metavar='PATH',
                        help='DAMSM image encoder weights (image_encoder100.pth; default: $XMC_DAMSM_IMAGE_ENCODER)')
    parser.add_argument('--text_encoder', type=str, default=None, metavar='PATH',
                        help='RNN presets: text encoder state dict (default: TEXT.ENCODER_DIR); SBERT presets: the model directory')
    parser.add_argument('--data_dir', type=str, default='', help='dataset root with captions.pickle, for --captions with an RNN preset')
    parser.add_argument('--k', type=int, default=100, help='candidates per image, the own caption included')
    parser.add_argument('--splits', type=int, default=10)
    parser.add_argument('--seed', type=int, default=0)
    parser.add_argument('--batch', type=int, default=100)
    parser.add_argument('--gpu', dest='gpu_id', type=int, default=0)
    return parser.parse_args(argv)


def _check_args(args):
    """everything that can be refused before a device is touched; -> the sorted image files"""
    from xmc_gan.config.gan import cfg, cfg_from_file
    from xmc_gan_amd.evaluate import resolve_weights
    from xmc_gan_amd.fid import list_images
    if bool(args.captions) == bool(args.token_ids):
        raise SystemExit('give exactly one caption source: --captions FILE or --token_ids FILE')
    if args.per_caption < 1 or args.k < 2 or args.splits < 1 or args.batch < 1:
        raise SystemExit('--per_caption, --splits and --batch must be >= 1 and --k >= 2')
    if not os.path.isdir(args.images):
        raise SystemExit(f'{args.images} is not a directory')
    files = list_images(args.images)
    if not files:
        raise SystemExit(f'{args.images} holds no image (.png / .jpg / .jpeg)')
    args.image_encoder = resolve_weights(args.image_encoder, 'XMC_DAMSM_IMAGE_ENCODER', '--image_encoder', refusal='the DAMSM image encoder weights are needed')
    cfg_from_file(args.cfg)
    if args.token_ids and cfg.TEXT.ENCODER_NAME != 'RNN':
        raise SystemExit(f'--token_ids feeds the RNN encoder; TEXT.ENCODER_NAME is {cfg.TEXT.ENCODER_NAME} (use --captions)')
    for what, path in (('--captions', args.captions), ('--token_ids', args.token_ids)):
        if path and not os.path.isfile(path):
            raise SystemExit(f'{what}: {path} is not a file')
    if cfg.TEXT.ENCODER_NAME == 'RNN' and args.text_encoder is not None and not os.path.isfile(args.text_encoder):
        raise SystemExit(f'--text_encoder: {args.text_encoder} is not a file')
    return files


def main(argv=None):
    args = parse_args(argv)
    files = _check_args(args)
    import torch
    from xmc_gan import sample
    from xmc_gan.config.gan import cfg
    from xmc_gan_amd import rprecision as RP
    from xmc_gan_amd.fid import decoded_batches
    args.synthetic, args.sbert_dir = 0, (args.text_encoder or '') if cfg.TEXT.ENCODER_NAME == 'SBERT' else ''
    tokens, lens, lines = sample._load_captions(args)
    n, K = len(lines), args.per_caption
    if len(files) != n * K:
        raise SystemExit(f'{args.images} holds {len(files)} images, {n} captions x --per_caption {K} = {n * K} were expected')
    if not torch.cuda.is_available():
        raise RuntimeError('xmc_gan/rprecision.py scores images on an MI355X (HIP kernels only)')
    torch.cuda.set_device(args.gpu_id)
    device = torch.device('cuda', args.gpu_id)
    torch.manual_seed(args.seed)
    try:
        image_encoder = RP.load_image_encoder(args.image_encoder, None, device)
        text_encoder = sample._text_encoder(args, device)
    except (ImportError, ValueError) as e:
        raise SystemExit(str(e))
    dim = cfg.TEXT.EMBEDDING_DIM
    if dim != image_encoder.nef:
        raise SystemExit(f"the text encoder's sentence codes have {dim} entries (TEXT.EMBEDDING_DIM), the image encoder's {image_encoder.nef}")
    sents = []
    with torch.no_grad():
        for i in range(0, n, args.batch):
            sents.append(text_encoder(tokens[i:i + args.batch], lens[i:i + args.batch])[1].detach().float())
    rp = RP.RPrecision(args.k, args.splits, args.seed)
    codes = torch.empty((n * K, image_encoder.nef), dtype=torch.float32, device=device)
    for idx, u8 in decoded_batches(files, args.batch):       # (the files of a batch that share a size go through the encoder together)
        codes[torch.tensor(idx, device=device)] = image_encoder.encode_u8(u8)[1]
    rp.update(codes, torch.cat(sents), torch.arange(n).repeat_interleave(K))
    try:
        result = rp.finalize()
    except ValueError as e:
        raise SystemExit(str(e))
    print(json.dumps(result))
    return result


if __name__ == '__main__':
    main()
