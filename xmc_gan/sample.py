"""Images from a trained generator: checkpoint + captions in, PNGs out.

    python xmc_gan/sample.py --cfg xmc_gan/cfg/<preset>.yml --checkpoint <netG_*.pth | netG_ema_*.pth> --out DIR
                             (--captions FILE | --token_ids FILE.npy | --synthetic N) [--n_per_caption K --seed S --truncation PSI]
                             [--best_of M --netD netD_*.pth] [--walk N] [--interp_sent N] [--grid_max N] [--no_png]
                             [--fid_against DIR_OR_NPZ --fid_inception PATH] [--prdc_against DIR_OR_FEATURES_NPZ [--prdc_k K]]
                             [--rprecision --damsm_image_encoder PATH] [--clip_score --clip_dir PATH [--clip_max_tokens N]]
                             [--kid_against DIR_OR_FEATURES_NPZ [--kid_subsets S --kid_subset_size M]] [--inception_score [--is_splits S]]

Writes ``<out>/<caption index:05d>_<k>.png`` (K images per caption), ``<out>/grid.png`` (the first ``--grid_max`` of them, every image min-max scaled
on its own like the trainer's sample grids), ``<out>/captions.txt`` and ``<out>/manifest.json``.  The generator runs on the HIP kernels of
``xmc_gan_amd`` in evaluation mode; the images are converted to uint8 on the device (``ops.image_to_u8`` / ``ops.image_grid_u8``), copied
to the host once per batch and PNG-encoded by a small thread pool.  The noise comes from a seeded CPU generator
(``xmc_gan_amd.infer.truncated_noise``), so the same arguments give the same files.  INTEGRATION.md section 3.3 has the details.
"""
import os
import sys

PROJ_DIR = os.path.abspath(os.path.join(os.path.dirname(os.path.realpath(__file__)), os.pardir))
if PROJ_DIR not in sys.path:
    sys.path.append(PROJ_DIR)

import argparse
import json
import pickle

import numpy as np
import torch

from xmc_gan.config.gan import cfg, cfg_from_file
from xmc_gan.dataset import sent_to_index
from xmc_gan.train_gan import _DISC_ARCH, _GEN_ARCH, SyntheticCOCO, build_text_encoder
from xmc_gan.utils.visual import PngPool
from xmc_gan_amd import ops
from xmc_gan_amd.evaluate import MetricSuite, image_set_kind, load_model, resolve_weights
from xmc_gan_amd.infer import Sampler, slerp, truncated_noise


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Sample images from a trained XMC-GAN / DF-GAN generator')
    parser.add_argument('--cfg', type=str, required=True, help='the preset the checkpoint was trained with')
    parser.add_argument('--checkpoint', type=str, required=True, help='generator state dict: netG_<epoch>.pth or netG_ema_<epoch>.pth')
    parser.add_argument('--out', type=str, required=True, help='output directory (created)')
    # captions: exactly one source
    parser.add_argument('--captions', type=str, default='', metavar='FILE',
                        help="one sentence per line, tokenised with the vocabulary (w2i) of <data_dir>/captions.pickle")
    parser.add_argument('--token_ids', type=str, default='', metavar='FILE', help='.npy int64 [n, TEXT.MAX_LENGTH] token ids, 0-padded')
    parser.add_argument('--synthetic', type=int, default=0, metavar='N', help="N of the trainer's synthetic captions")
    parser.add_argument('--data_dir', type=str, default='', help='dataset root (default: <repo>/data/<DATASET_NAME>)')
    # sampling and model
    parser.add_argument('--n_per_caption', type=int, default=1, metavar='K')
    parser.add_argument('--seed', type=int, default=100)
    parser.add_argument('--truncation', type=float, default=None, metavar='PSI',
                        help='truncation trick: noise entries with |z| > PSI are drawn again (default: plain normal noise)')
    parser.add_argument('--bs', type=int, default=-1, help='images per forward (default: TRAIN.BATCH_SIZE)')
    parser.add_argument('--imsize', type=int, default=-1)
    parser.add_argument('--precision', type=str, default=None, choices=['bf16', 'f16', 'fp32'])
    parser.add_argument('--gpu', dest='gpu_id', type=int, default=0)
    parser.add_argument('--text_encoder', type=str, default=None, metavar='PATH', help='text encoder state dict (default: TEXT.ENCODER_DIR)')
    parser.add_argument('--sbert_dir', type=str, default='', metavar='PATH',
                        help='TEXT.ENCODER_NAME SBERT: the RoBERTa model directory of the sentence encoder (default: $XMC_SBERT_DIR)')
    # scoring
    parser.add_argument('--fid_against', type=str, default='', metavar='DIR_OR_NPZ',
                        help='score the sampled images: FID against an image directory or an .npz statistics file -> manifest "fid"')
    parser.add_argument('--fid_inception', type=str, default='', metavar='PATH',
                        help='FID Inception weights for --fid_against (the pt_inception-2015-12-05-*.pth state dict; default: $XMC_FID_INCEPTION)')
    parser.add_argument('--prdc_against', type=str, default='', metavar='DIR_OR_FEATURES_NPZ',
                        help='score the sampled images: precision / recall / density / coverage against an image directory or an .npz feature '
                             'file (xmc_gan/prdc.py --save_features) -> manifest "prdc"; takes --fid_inception')
    parser.add_argument('--prdc_k', type=int, default=5, metavar='K', help='--prdc_against: nearest neighbours (1..16)')
    parser.add_argument('--kid_against', type=str, default='', metavar='DIR_OR_FEATURES_NPZ',
                        help='Kernel Inception Distance of the sampled images against an image directory or an .npz feature file '
                             '-> manifest "kid"; takes --fid_inception.  The subsets are drawn with --seed (default 100): '
                             'xmc_gan/kid.py gives the same value with --seed set to that')
    parser.add_argument('--kid_subsets', type=int, default=100, metavar='S', help='--kid_against: the number of subsets')
    parser.add_argument('--kid_subset_size', type=int, default=1000, metavar='M', help='--kid_against: rows per side of a subset (at most)')
    parser.add_argument('--inception_score', action='store_true',
                        help='Inception Score of the sampled images -> manifest "inception_score"; takes --fid_inception')
    parser.add_argument('--is_splits', type=int, default=10, metavar='S', help='--inception_score: consecutive parts the mean and its spread are taken over')
    parser.add_argument('--rprecision', action='store_true',
                        help='score the sampled images: R-precision against their captions (RNN presets) -> manifest "r_precision"')
    parser.add_argument('--damsm_image_encoder', type=str, default='', metavar='PATH',
                        help="DAMSM image encoder weights for --rprecision (image_encoder100.pth; default: $XMC_DAMSM_IMAGE_ENCODER)")
    parser.add_argument('--clip_score', action='store_true',
                        help='score the sampled images: CLIPScore against the sentences of --captions -> manifest "clip_score"')
    parser.add_argument('--clip_dir', type=str, default='', metavar='PATH',
                        help='--clip_score: a Hugging Face CLIPModel directory, e.g. a copy of openai/clip-vit-base-patch32 (default: $XMC_CLIP_DIR)')
    parser.add_argument('--clip_max_tokens', type=int, default=64, metavar='N',
                        help="--clip_score: the longest sequence CLIPScore's towers take (default 64: ViT-B/32 at a text context of 64, today's scores).  77 or more gives CLIP's own text context of 77 tokens and admits ViT-B/16 (197 tokens) and ViT-L/14 (257; 577 at 336 px); at most 1024")
    parser.add_argument('--rp_k', type=int, default=100, metavar='K', help='--rprecision: candidates per image, the own caption included')
    parser.add_argument('--rp_splits', type=int, default=10, metavar='S', help='--rprecision: parts the mean and its spread are taken over')
    # reranking
    parser.add_argument('--best_of', type=int, default=0, metavar='M',
                        help="draw M images per caption and keep the K the discriminator's conditional logit ranks highest (needs --netD)")
    parser.add_argument('--netD', type=str, default='', metavar='PATH', help='discriminator state dict: netD_<epoch>.pth')
    # latent walks
    parser.add_argument('--walk', type=int, default=0, metavar='N',
                        help="per caption, N frames on the spherical interpolation between its first two noises -> <idx>_walk.png")
    parser.add_argument('--interp_sent', type=int, default=0, metavar='N',
                        help='for the caption pairs (0,1), (2,3), ...: N frames between the two sentence embeddings at fixed noise '
                             '-> <idx>_<idx+1>_interp.png (DF_GEN only)')
    parser.add_argument('--grid_max', type=int, default=256, metavar='N', help='grid.png shows the first N images (0: no grid)')
    parser.add_argument('--no_png', action='store_true', help='skip the per-image PNGs (grid, captions and manifest are still written)')
    return parser.parse_args(argv)


def _check_args(args):
    """everything that can be refused from the arguments and the cfg alone, before a device is touched"""
    if sum(map(bool, (args.captions, args.token_ids, args.synthetic > 0))) != 1:
        raise SystemExit('give exactly one caption source: --captions FILE, --token_ids FILE or --synthetic N')
    if args.n_per_caption < 1 or args.best_of < 0 or args.walk < 0 or args.interp_sent < 0 or args.synthetic < 0 or args.grid_max < 0:
        raise SystemExit('--n_per_caption must be >= 1; --best_of, --walk, --interp_sent, --synthetic and --grid_max >= 0')
    if args.best_of and not args.netD:
        raise SystemExit('--best_of ranks by the discriminator: give its weights with --netD netD_<epoch>.pth')
    if args.best_of and args.best_of < args.n_per_caption:
        raise SystemExit(f'--best_of {args.best_of} draws fewer images than --n_per_caption {args.n_per_caption} keeps')
    if args.truncation is not None and not args.truncation > 0:
        raise SystemExit('--truncation must be > 0')
    if args.walk == 1 or args.interp_sent == 1:
        raise SystemExit('--walk / --interp_sent need at least 2 frames')
    if args.walk and max(args.n_per_caption, args.best_of) < 2:
        raise SystemExit("--walk goes from a caption's first noise to its second: ask for --n_per_caption 2 (or more)")
    for flag, path, holds in (('--fid_against', args.fid_against, 'statistics'), ('--prdc_against', args.prdc_against, 'feature'),
                              ('--kid_against', args.kid_against, 'feature')):
        if path:
            if image_set_kind(path) is None:
                raise SystemExit(f'{flag}: {path} is neither an image directory nor an .npz {holds} file')
            if flag == '--prdc_against' and not 1 <= args.prdc_k <= 16:
                raise SystemExit(f'--prdc_k: {args.prdc_k}; 1 <= K <= 16 expected')
            if flag == '--kid_against' and (args.kid_subsets < 1 or args.kid_subset_size < 2):
                raise SystemExit(f'--kid_subsets {args.kid_subsets} / --kid_subset_size {args.kid_subset_size}: S >= 1 and M >= 2 expected')
            args.fid_inception = resolve_weights(args.fid_inception, 'XMC_FID_INCEPTION', '--fid_inception',
                                                 refusal=f'{flag} needs the FID Inception weights')
    if args.inception_score:
        if args.is_splits < 1:
            raise SystemExit(f'--is_splits: {args.is_splits}; at least one part expected')
        args.fid_inception = resolve_weights(args.fid_inception, 'XMC_FID_INCEPTION', '--fid_inception',
                                             refusal='--inception_score needs the FID Inception weights')
    if args.rprecision:
        args.damsm_image_encoder = resolve_weights(args.damsm_image_encoder, 'XMC_DAMSM_IMAGE_ENCODER', '--damsm_image_encoder',
                                                   refusal='--rprecision needs the DAMSM image encoder weights')
        if args.rp_k < 2 or args.rp_splits < 1:
            raise SystemExit('--rp_k must be >= 2 and --rp_splits >= 1')
    if args.clip_score:
        args.clip_dir = args.clip_dir or os.environ.get('XMC_CLIP_DIR', '')
        if not os.path.isfile(os.path.join(args.clip_dir, 'config.json')):
            raise SystemExit(f'--clip_score needs a CLIP model directory: --clip_dir PATH or XMC_CLIP_DIR (got {args.clip_dir!r})')
        if not args.captions:
            raise SystemExit('--clip_score compares the images with the sentences of --captions FILE; --token_ids and --synthetic hold no text')
    cfg_from_file(args.cfg)
    if args.imsize != -1:
        cfg.IMG.SIZE = args.imsize
    if args.bs != -1:
        cfg.TRAIN.BATCH_SIZE = args.bs
    if cfg.TRAIN.BATCH_SIZE < 1:
        raise SystemExit('--bs must be >= 1')
    if args.rprecision and cfg.TEXT.ENCODER_NAME != 'RNN':
        raise SystemExit(f"--rprecision pairs the DAMSM image encoder with the RNN caption encoder's sentence codes; TEXT.ENCODER_NAME is "
                         f'{cfg.TEXT.ENCODER_NAME} (score the PNGs with xmc_gan/rprecision.py and a DAMSM text encoder instead)')
    if args.interp_sent and cfg.GEN.ENCODER_NAME != 'DF_GEN':
        raise SystemExit(f'--interp_sent moves the sentence embedding alone, which describes the caption only for a generator that ignores '
                         f'the word embeddings (DF_GEN); GEN.ENCODER_NAME is {cfg.GEN.ENCODER_NAME}')
    if args.token_ids and cfg.TEXT.ENCODER_NAME != 'RNN':
        raise SystemExit(f'--token_ids feeds the RNN encoder; TEXT.ENCODER_NAME is {cfg.TEXT.ENCODER_NAME} (use --captions)')
    for what, path in (('--checkpoint', args.checkpoint), ('--netD', args.netD), ('--captions', args.captions),
                       ('--token_ids', args.token_ids), ('--text_encoder', args.text_encoder)):
        if path and not os.path.isfile(path):
            raise SystemExit(f'{what}: {path} is not a file')


def _load_captions(args):
    """-> (captions for the text encoder: int64 [n, MAX_LENGTH] token ids or a list of sentences; lengths [n]; one printable line each).
    Host work only.  None for --synthetic (drawn once the device is known, like the trainer does)."""
    T = cfg.TEXT.MAX_LENGTH
    if args.token_ids:
        ids = np.load(args.token_ids)
        if ids.ndim != 2 or ids.shape[1] != T or ids.dtype.kind not in 'iu' or ids.shape[0] < 1:
            raise SystemExit(f'--token_ids: integer [n, {T}] expected, got {ids.dtype} {ids.shape}')
        ids = torch.from_numpy(ids.astype(np.int64))
        lens = (ids != 0).sum(1)
        if int(lens.min()) < 1 or bool(((ids == 0).cumsum(1) > 0)[:, :-1].logical_and(ids[:, 1:] != 0).any()):
            raise SystemExit('--token_ids: every row needs at least one token, and 0 only as padding after the last one')
        if int(ids.max()) >= cfg.TEXT.VOCA_SIZE or int(ids.min()) < 0:
            raise SystemExit(f'--token_ids: ids must be in [0, {cfg.TEXT.VOCA_SIZE})')
        return ids, lens, [' '.join(str(t) for t in row[:n]) for row, n in zip(ids.tolist(), lens.tolist())]
    if args.captions:
        with open(args.captions) as f:
            sents = [line.strip() for line in f if line.strip()]
        if not sents:
            raise SystemExit(f'--captions: {args.captions} holds no sentence')
        if cfg.TEXT.ENCODER_NAME != 'RNN':                # the sentence encoder takes the sentences themselves (SentTextDataset)
            return sents, torch.tensor([len(s.split(' ')) for s in sents]), sents
        path = os.path.join(args.data_dir or f'{PROJ_DIR}/data/{cfg.DATASET_NAME}', 'captions.pickle')
        if not os.path.isfile(path):
            raise SystemExit(f'--captions needs the vocabulary of {path} (--data_dir)')
        with open(path, 'rb') as f:
            w2i = pickle.load(f)[3]
        try:
            rows = [sent_to_index(w2i, s, T) for s in sents]
        except ValueError as e:
            raise SystemExit(f'--captions: {e}')
        return torch.from_numpy(np.stack([r for r, _ in rows])), torch.tensor([n for _, n in rows]), sents
    return None


def _text_encoder(args, device):
    """the trainer's encoder for this cfg (random weights come from torch.manual_seed(--seed) in main()), or --text_encoder's state dict"""
    enc, has_weights = build_text_encoder(device, args.seed, args.synthetic > 0, args.sbert_dir, weights=args.text_encoder)
    if not has_weights and args.synthetic <= 0:
        print('sample.py: no text encoder weights (--text_encoder / TEXT.ENCODER_DIR): the encoder is randomly initialised', file=sys.stderr)
    return enc


def _row_grid(x8_frames, path):
    """N frames as one grid row, scaled per image like every sample grid"""
    from PIL import Image
    Image.fromarray(ops.image_grid_u8(x8_frames, nrow=x8_frames.size(0)).cpu().numpy()).save(path)


_SCORES = {     # metric of MetricSuite.results(): (the flag that asked for it, its printed line, its manifest key)
    'FID': ('--fid_against', 'FID: {FID}', 'fid'),
    'PRDC': ('--prdc_against', 'precision: {precision} recall: {recall} density: {density} coverage: {coverage} (k={k}, n={n_real}/{n_fake})', 'prdc'),
    'R-precision': ('--rprecision', 'R-precision: {r_precision} +- {std} (k={k}, n={n})', 'r_precision'),
    'KID': ('--kid_against', 'KID: {kid} +- {std} (subsets={subsets}, size={subset_size}, n={n_real}/{n_fake})', 'kid'),
    'IS': ('--inception_score', 'IS: {inception_score} +- {std} (splits={splits}, n={n})', 'inception_score'),
    'CLIPScore': ('--clip_score', 'CLIPScore: {clip_score} +- {std} (n={n}, model={model})', 'clip_score'),
}


def main(argv=None):
    args = parse_args(argv)
    _check_args(args)
    caps = _load_captions(args)
    if args.precision:
        ops.set_precision(args.precision)
    if not torch.cuda.is_available():
        raise RuntimeError('xmc_gan/sample.py needs an MI355X (HIP kernels only)')
    torch.cuda.set_device(args.gpu_id)
    device = torch.device('cuda', args.gpu_id)
    torch.manual_seed(args.seed)
    torch.cuda.manual_seed_all(args.seed)

    if caps is None:
        _, ids, lens = SyntheticCOCO(1, args.synthetic, 1, cfg.TEXT.MAX_LENGTH, args.seed, cfg.TEXT.VOCA_SIZE)._batch(0)
        caps = (ids, lens, [' '.join(str(t) for t in row[:n]) for row, n in zip(ids.tolist(), lens.tolist())])
    tokens, lens, lines = caps
    n, K = len(lines), args.n_per_caption
    M = args.best_of or K                                            # draws per caption
    bs = cfg.TRAIN.BATCH_SIZE

    text_encoder = _text_encoder(args, device)
    netG = _GEN_ARCH[cfg.GEN.ENCODER_NAME](cfg).to(device)
    netG.load_state_dict(torch.load(args.checkpoint, map_location=device))
    netG.eval().requires_grad_(False)
    netD = None
    if args.netD:
        netD = _DISC_ARCH[cfg.DISC.ENCODER_NAME](cfg, is_disc=True).to(device)
        netD.load_state_dict(torch.load(args.netD, map_location=device))
        netD.eval().requires_grad_(False)
    sampler = Sampler(netG, netD, separate=cfg.DISC.SEPERATE)

    # every caption's embeddings, `bs` captions per encoder call
    words, sents, masks = [], [], []
    with torch.no_grad():
        for i in range(0, n, bs):
            w_, s_, m_ = text_encoder(tokens[i:i + bs], lens[i:i + bs])
            words.append(w_.detach()), sents.append(s_.detach()), masks.append(m_)
    words, sents, masks = torch.cat(words), torch.cat(sents), torch.cat(masks)

    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'captions.txt'), 'w') as f:
        f.write(''.join(f'{line}\n' for line in lines))
    noise = truncated_noise(n * M, cfg.TRAIN.NOISE_DIM, args.seed, args.truncation)          # rows c*M .. c*M + M - 1: caption c
    S = cfg.IMG.SIZE
    n_grid = min(n * K, args.grid_max)
    kept = torch.empty((n_grid, S, S, 8), dtype=ops.act_dtype(), device=device) if n_grid else None      # the grid's images, engine layout
    images, pool = [], (None if args.no_png else PngPool())
    if args.rprecision:
        try:
            load_model('damsm', args.damsm_image_encoder, device)
        except (ImportError, ValueError) as e:
            raise SystemExit(f'--damsm_image_encoder: {e}')
    # the sampled images are scored from the device, as the bytes of the PNGs (xmc_gan_amd/evaluate.py: one pass serves every metric asked for)
    more = {}                                                        # (KID and the Inception Score: no argument at all while both are off)
    if args.kid_against:
        more.update(kid=True, kid_subsets=args.kid_subsets, kid_subset_size=args.kid_subset_size, kid_seed=args.seed)
    if args.inception_score:
        more.update(inception_score=args.is_splits)
    if args.clip_score:
        tokens = {} if args.clip_max_tokens == 64 else {'max_tokens': args.clip_max_tokens}
        more.update(clip_dir=args.clip_dir, **{'clip_' + k: v for k, v in tokens.items()})
        try:
            load_model('clip', args.clip_dir, device, **tokens)
        except (ImportError, ValueError, NotImplementedError) as e:
            raise SystemExit(f'--clip_dir: {e}')
    suite = MetricSuite(device, args.fid_inception if (args.fid_against or args.prdc_against or args.kid_against or args.inception_score) else '', args.prdc_k if args.prdc_against else 0,
                        args.damsm_image_encoder if args.rprecision else '', text_encoder, args.rp_k, args.rp_splits, args.seed,
                        fid=bool(args.fid_against), **more)
    for metric, why in suite.why.items():
        raise SystemExit(f'{_SCORES[metric][0]}: {why}')
    suite.real_from_path(args.fid_against, args.prdc_against, bs, **({'kid_path': args.kid_against} if args.kid_against else {}))
    cap_step = max(1, bs // M)                                       # captions per batch: about `bs` forwards' worth of images
    try:
        for c0 in range(0, n, cap_step):
            c1 = min(n, c0 + cap_step)
            nc = c1 - c0
            rep = lambda t, r: t[c0:c1].repeat_interleave(r, dim=0)          # noqa: E731
            z = noise[c0 * M:c1 * M]
            if args.best_of:
                u8, sc, _, x8 = sampler.best_of(M, K, z, sents[c0:c1], words[c0:c1], masks[c0:c1], micro_batch=bs, keep_engine=True)
                u8, sc = u8.reshape((nc * K,) + tuple(u8.shape[2:])), sc.reshape(-1).tolist()
            else:
                x8 = sampler.engine_images(z, rep(sents, K), rep(words, K), rep(masks, K))
                u8, sc = ops.image_to_u8(x8), None
            if c0 * K < n_grid:
                kept[c0 * K:min(n_grid, c1 * K)] = x8[:n_grid - c0 * K]
            pairing = torch.arange(nc).repeat_interleave(K)          # image r of the batch was made from caption r // K
            if args.clip_score:
                suite.update_fake(u8, sents[c0:c1], pairing, captions=lines[c0:c1])
            else:
                suite.update_fake(u8, sents[c0:c1], pairing)
            host = u8.cpu().numpy()                                  # one copy per batch: 3 bytes per pixel
            for r in range(nc * K):
                c, k = c0 + r // K, r % K
                rec = dict(caption=c, k=k, file=None if args.no_png else f'{c:05d}_{k}.png')
                if sc is not None:
                    rec['score'] = sc[r]
                images.append(rec)
                if pool is not None:
                    pool.put(host[r], os.path.join(args.out, rec['file']))
            if args.walk:
                t = torch.linspace(0.0, 1.0, args.walk)
                for c in range(c0, c1):
                    frames = slerp(noise[c * M].expand(args.walk, -1), noise[c * M + 1].expand(args.walk, -1), t)
                    e = lambda v: v[c:c + 1].expand(args.walk, *v.shape[1:])          # noqa: E731
                    _row_grid(sampler.engine_images(frames, e(sents), e(words), e(masks)), os.path.join(args.out, f'{c:05d}_walk.png'))
    finally:
        if pool is not None:
            pool.close()
    walks = [f'{c:05d}_walk.png' for c in range(n)] if args.walk else []
    interps = []
    if args.interp_sent:
        t = torch.linspace(0.0, 1.0, args.interp_sent, device=device)[:, None]
        for c in range(0, n - 1, 2):
            s_ = (1.0 - t) * sents[c:c + 1].float() + t * sents[c + 1:c + 2].float()
            z = noise[c * M].expand(args.interp_sent, -1)
            e = lambda v: v[c:c + 1].expand(args.interp_sent, *v.shape[1:])              # noqa: E731
            interps.append(f'{c:05d}_{c + 1:05d}_interp.png')
            _row_grid(sampler.engine_images(z, s_, e(words), e(masks)), os.path.join(args.out, interps[-1]))
    grid = None
    if kept is not None:
        from PIL import Image
        grid = 'grid.png'
        Image.fromarray(ops.image_grid_u8(kept).cpu().numpy()).save(os.path.join(args.out, grid))
    scores = {}
    for metric, values, why in suite.results():
        flag, line, key = _SCORES[metric]
        if values is None:
            raise SystemExit(f'{flag}: {"a covariance needs at least two sampled images" if metric == "FID" else why}')
        print(line.format(**values))
        scores[key] = values
    manifest = dict(checkpoint=os.path.abspath(args.checkpoint), netD=os.path.abspath(args.netD) if args.netD else None,
                    cfg=os.path.abspath(args.cfg), config_name=cfg.CONFIG_NAME, generator=cfg.GEN.ENCODER_NAME, img_size=S,
                    seed=args.seed, precision=ops.precision(), truncation=args.truncation, n_per_caption=K, best_of=args.best_of or None,
                    captions=n, fid=scores.pop('fid', {}).get('FID'), grid=grid, grid_images=n_grid, walks=walks, interps=interps, images=images)
    manifest.update({key: scores[key] for key in ('r_precision', 'prdc', 'kid', 'inception_score', 'clip_score') if key in scores})     # (only when asked for, in the order of before)
    with open(os.path.join(args.out, 'manifest.json'), 'w') as f:
        json.dump(manifest, f, indent=1)
    torch.cuda.synchronize()
    main.last_sampler = sampler          # (for callers that drive main() in-process: the tests rebuild the images from these)
    main.last_inputs = dict(noise=noise, sent_embs=sents, words_embs=words, mask=masks)
    return manifest


if __name__ == '__main__':
    main()
