"""cfg-driven XMC-GAN / DF-GAN trainer on MI355X -- drop-in for the reference entrypoint
(``python xmc_gan/train_gan.py --cfg xmc_gan/cfg/<preset>.yml [--gpu --seed --resume_epoch --log_type --bs --imsize]``).

Same flags, registries (``_GEN_ARCH`` / ``_DISC_ARCH``), helper names (``weight_init``, ``make_labels``,
``cosine_scores``, ``sent_loss``, ``img_loss``, ``train``, ``eval``) and the same arithmetic per iteration
as the reference loop (train_gan.py:174-293).  Every pass over an activation-, image- or parameter-sized tensor runs in a
hand-written HIP kernel through ``xmc_gan_amd``; what is left to ATen is batch-sized glue ([B], [B,cond] or [B,4,4,C]
tensors: the concatenations that build COND_DNET's input, slices of the padded logits, ``-mean(logit)``, the threshold
arithmetic of ``make_labels``) and the collectives.  Parity: ``--precision fp32`` reproduces the CPU reference to 1e-3
(measured ~1e-6); the default bf16 mode is checked against the quantisation-aware oracle and costs ~1e-2 on the losses
against the f32 reference (tests/test_models_gpu.py states both).  Extras that the reference lacks: ``--synthetic`` COCO-shaped random data
(the COCO pickles / DAMSM weights are not redistributable), ``--precision``, and one-process-per-GPU data
parallelism when launched under ``torch.distributed.run`` (gradient all-reduce + optional all-gathered
contrastive negatives, ``--gather_negatives``).
"""
import contextlib
import os
import sys

PROJ_DIR = os.path.abspath(os.path.join(os.path.dirname(os.path.realpath(__file__)), os.pardir))
if PROJ_DIR not in sys.path:
    sys.path.append(PROJ_DIR)

import argparse
import collections
import random
import time
import types

import numpy as np
import torch

from xmc_gan.config.gan import cfg, cfg_from_file
from xmc_gan.model.df_gan import NetG as DF_GEN, NetD as DF_DISC
from xmc_gan.model.df_concept_gan import InNetG as CONCEPT_IN_DF_GEN, OutNetG as CONCEPT_OUT_DF_GEN, NetD as CONCEPT_NETD
from xmc_gan.dataset import SentTextDataset, WordTextDataset, test_transform, train_transform
from xmc_gan.model.concept_gan import InNetG as CONCEPT_INATTN_GEN, OutNetG as CONCEPT_OUTATTN_GEN
from xmc_gan.model.encoder import RNN_ENCODER, SBERT_ENCODER
from xmc_gan.utils.logger import setup_logger
from xmc_gan.utils.miscc import count_params
from xmc_gan.utils.visual import ScalarLog, fid_between, flush_saves, save_image, save_image_async, to_uint8_hwc
from xmc_gan_amd import ops, parallel
from xmc_gan_amd.augment import DiffAugment, parse_policy
from xmc_gan_amd.evaluate import MetricSuite, resolve_weights
from xmc_gan_amd.graph import CaptureFailed, GraphedIteration
from xmc_gan_amd.optim import HipAdam, ParamEMA
from xmc_gan_amd.vgg import VGG19Features, VGGContrast, resolve_vgg_weights

_GEN_ARCH = {"DF_GEN": DF_GEN, "CONCEPT_IN_DF_GEN": CONCEPT_IN_DF_GEN, "CONCEPT_OUT_DF_GEN": CONCEPT_OUT_DF_GEN,
             # word-attention generators of model/concept_gan.py; upstream keeps these two names commented out (train_gan.py:44)
             "CONCEPT_OUTATTN_GEN": CONCEPT_OUTATTN_GEN, "CONCEPT_INATTN_GEN": CONCEPT_INATTN_GEN}
_DISC_ARCH = {"DF_DISC": DF_DISC, "CONCEPT_NETD": CONCEPT_NETD}
_TEXT_DATASET = {"WORD": WordTextDataset, "SENT": SentTextDataset}
_TEXT_ARCH = {"RNN": RNN_ENCODER, "SBERT": SBERT_ENCODER}


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Train XMC-GAN')
    parser.add_argument('--cfg', type=str, default='xmc_gan/cfg/df_gan_sbert_seperate.yml')
    parser.add_argument('--gpu', dest='gpu_id', type=int, default=0)
    parser.add_argument('--seed', type=int, default=100)
    parser.add_argument('--resume_epoch', type=int, default=0)
    parser.add_argument('--log_type', type=str, default='tb')
    parser.add_argument('--bs', type=int, default=-1)
    parser.add_argument('--imsize', type=int, default=-1)
    # additions
    parser.add_argument('--synthetic', type=int, default=0, metavar='N',
                        help='train on N COCO-shaped random batches per epoch instead of data/<DATASET_NAME>')
    parser.add_argument('--max_epoch', type=int, default=-1)
    parser.add_argument('--data_dir', type=str, default='', help='dataset root (default: <repo>/data/<DATASET_NAME>)')
    parser.add_argument('--output_dir', type=str, default='', help='run directory (default: <repo>/output/<name>)')
    parser.add_argument('--precision', type=str, default=None, choices=['bf16', 'f16', 'fp32'])
    parser.add_argument('--gather_negatives', action='store_true',
                        help='data parallel: all-gather embeddings so the contrastive losses see world*batch negatives')
    parser.add_argument('--graph', type=int, default=1,
                        help='1 (default): replay the G+D iteration as hipGraphs (two eager warm-up iterations, then one capture per '
                             'N_CRITIC phase); 0: launch every kernel from Python (host-bound: ~55 ms per iteration whatever the batch)')
    parser.add_argument('--log_each_step', type=int, default=0,
                        help="1: the reference's loss line after EVERY generator step (one host synchronisation per iteration); default: "
                             'at the first step and every LOG_INTERVAL steps')
    parser.add_argument('--ema_decay', type=float, default=0.0,
                        help='> 0: keep an exponential moving average of the generator weights on the device (typical: 0.999 / 0.9999); '
                             'the per-epoch sample grid, eval() and netG_ema_<epoch>.pth use it.  0 (default): off')
    parser.add_argument('--ema_start', type=int, default=0,
                        help='generator steps before the averaging starts: until then the average is a copy of the weights')
    parser.add_argument('--fid_inception', type=str, default='', metavar='PATH',
                        help="FID Inception weights (the pt_inception-2015-12-05-*.pth state dict of pytorch_fid): eval() scores on this "
                             "project's kernels (default: $XMC_FID_INCEPTION; without either, pytorch_fid if it is installed)")
    parser.add_argument('--prdc', type=int, default=0, metavar='K',
                        help='> 0: eval() also reports improved precision / recall and density / coverage with K nearest neighbours (typical: '
                             '5), from the Inception features it extracts for FID (needs --fid_inception or XMC_FID_INCEPTION).  0 (default): off')
    parser.add_argument('--kid', action='store_true',
                        help='eval() also reports the Kernel Inception Distance (mean +- spread over subsets) from the same Inception '
                             'features (needs --fid_inception or XMC_FID_INCEPTION)')
    parser.add_argument('--kid_subsets', type=int, default=100, metavar='S', help='--kid: the number of subsets (default 100)')
    parser.add_argument('--kid_subset_size', type=int, default=1000, metavar='M',
                        help='--kid: rows per side of a subset (default 1000; at most the number of images scored)')
    parser.add_argument('--inception_score', type=int, nargs='?', const=10, default=0, metavar='SPLITS',
                        help='eval() also reports the Inception Score of the generated images over SPLITS consecutive parts (default 10 when '
                             'the flag is given without a value; needs --fid_inception or XMC_FID_INCEPTION).  0: off')
    parser.add_argument('--damsm_image_encoder', type=str, default='', metavar='PATH',
                        help="DAMSM image encoder weights (image_encoder100.pth of AttnGAN's DAMSM archive): eval() also reports R-precision "
                             "(RNN presets; default: $XMC_DAMSM_IMAGE_ENCODER; without either, no R-precision)")
    parser.add_argument('--clip_dir', type=str, default='', metavar='PATH',
                        help='a Hugging Face CLIPModel directory (config.json, weights, tokenizer.json; e.g. a copy of '
                             'openai/clip-vit-base-patch32): eval() also reports CLIPScore of the generated images against their captions '
                             '(default: $XMC_CLIP_DIR; without either, no CLIPScore)')
    parser.add_argument('--clip_max_tokens', type=int, default=64, metavar='N',
                        help="--clip_dir: the longest sequence CLIPScore's towers take (default 64: ViT-B/32 at a text context of 64, today's scores).  77 or more gives CLIP's own text context of 77 tokens and admits ViT-B/16 (197 tokens) and ViT-L/14 (257; 577 at 336 px); at most 1024")
    parser.add_argument('--sbert_dir', type=str, default='', metavar='PATH',
                        help='TEXT.ENCODER_NAME SBERT: the RoBERTa model directory of the sentence encoder (config.json, weights, tokenizer '
                             'files; default: $XMC_SBERT_DIR).  Without it the SBERT presets run with --synthetic only')
    parser.add_argument('--diffaug', type=str, default='',
                        help="differentiable augmentation of every image the discriminator sees: comma list out of color, translation, "
                             "cutout (typical: all three).  '' (default): off")
    parser.add_argument('--vgg_weights', type=str, default='', metavar='PATH',
                        help="TRAIN.ENCODER_LOSS.VGG: torchvision's VGG-19 weights (the vgg19-dcbb9e9d.pth state dict) of the frozen network "
                             "behind the image-image contrastive term (default: $XMC_VGG19).  Without the switch nothing is loaded")
    parser.add_argument('--vgg_smooth', type=float, default=1.0, metavar='FLOAT',
                        help="weight of the VGG term in the generator's loss (the reference's yml schema has no SMOOTH.VGG; default 1.0)")
    parser.add_argument('--image_cache', type=str, default='', metavar='DIR',
                        help='train and evaluate from the uint8 image cache in DIR (built by xmc_gan/image_cache.py): the resized images '
                             'stay in device memory and a batch is one crop + flip + normalise launch instead of the PIL DataLoader')
    parser.add_argument('--caption_cache', type=str, default='', metavar='DIR',
                        help='take the text encoder\'s outputs from the caption-embedding cache in DIR (built by xmc_gan/caption_cache.py): '
                             'no text encoder is constructed, a batch is one gather launch over tables that stay in device memory')
    return parser.parse_args(argv)


def weight_init(m):
    """Kaiming-normal (fan_in, relu gain) for every conv / linear weight, zero bias (train_gan.py:65-69)."""
    if isinstance(m, (torch.nn.Conv2d, torch.nn.Linear)):
        torch.nn.init.kaiming_normal_(m.weight, mode='fan_in', nonlinearity='relu')
        if m.bias is not None:
            torch.nn.init.constant_(m.bias, 0)


# --------------------------------------------------------------------------------------- contrastive head
def cosine_scores(emb0, emb1):
    """[bs,D] x [bs,D] -> [bs,bs] cosine similarities (train_gan.py:85-91)."""
    return ops.cosine_scores(emb0, emb1)


def make_labels(batch_size, sent_embs, b_global, p=0.6):
    """Positive-pair weights for the contrastive losses (train_gan.py:72-83)."""
    labels = torch.eye(batch_size, device=sent_embs.device)
    if b_global:
        sim_mat = cosine_scores(sent_embs, sent_embs)
        sim_mat.fill_diagonal_(3)
        global_pos = (sim_mat > p) & (sim_mat < 3)
        num_pos = global_pos.sum(1).clamp_(min=1) + 1
        global_weight = cfg.TRAIN.SMOOTH.GLOBAL if (cfg.TRAIN.SMOOTH.GLOBAL != 0.) else torch.reciprocal(num_pos.float())
        labels = (labels + global_weight * global_pos).clamp_(max=1)   # [bs] weight broadcasts along columns
    return labels.detach()


def _info_nce(a, b, labels, b_global):
    if not b_global:
        inv_num_pos, lab = None, None                   # labels are the identity: kernel fast path
    elif cfg.TRAIN.SMOOTH.GLOBAL == 0.:
        inv_num_pos, lab = torch.full((labels.size(0),), 0.5, device=labels.device), labels.contiguous()
    else:
        inv_num_pos, lab = torch.reciprocal((labels > 0).sum(1).float()), labels.contiguous()
    return ops.contrastive(a, b, lab, inv_num_pos)


def sent_loss(imgs, txts, labels, b_global):
    """image-embedding <-> sentence-embedding symmetric InfoNCE without temperature (train_gan.py:93-115)."""
    return _info_nce(imgs, txts, labels, b_global)


def img_loss(real_imgs, fake_imgs, labels, b_global):
    """real-feature <-> fake-feature symmetric InfoNCE (train_gan.py:117-139)."""
    return _info_nce(real_imgs, fake_imgs, labels, b_global)


# --------------------------------------------------------------------------------------- one iteration
class StepOptions:
    """Engine-side switches of an iteration (not part of the reference cfg)."""

    def __init__(self, gather_negatives=False, graph=False, log_each_step=True, ema=None, diffaug=None, vgg=None, vgg_smooth=1.0):
        self.gather_negatives = gather_negatives
        self.vgg = vgg                        # xmc_gan_amd.vgg.VGGContrast: the frozen network of TRAIN.ENCODER_LOSS.VGG (None without the switch)
        self.vgg_smooth = vgg_smooth          # weight of the VGG term (--vgg_smooth; the reference's SMOOTH has no VGG entry)
        self.diffaug = diffaug                # xmc_gan_amd.augment.DiffAugment: netD sees augmented images only; train() refreshes its rows
        self.ema = ema                        # xmc_gan_amd.optim.ParamEMA of the generator: one update per applied generator step
        self.graph = graph                    # train(): replay the iteration as hipGraphs (xmc_gan_amd.graph.GraphedIteration)
        self.log_each_step = log_each_step    # train(): read the four logged losses back after every generator step


def _step(optimizer, scaler, ema=None):
    """optimizer.step(), with the dynamic loss scale only where there is one (IEEE-half mode): any torch.optim optimizer works
    in the bf16 / fp32 modes, as upstream's torch.optim.Adam does.  ``ema``: the weight average takes this step's weights -- inside
    HipAdam's kernel, or in a launch of its own after any other optimizer"""
    if ema is None:
        return optimizer.step(scaler=scaler) if scaler is not None else optimizer.step()
    if isinstance(optimizer, HipAdam):
        return optimizer.step(scaler=scaler, ema=ema)
    if scaler is not None:
        raise RuntimeError('a weight average under the dynamic loss scale needs HipAdam (the skipped steps are known on the device only)')
    out = optimizer.step()
    ema.update()
    return out


def _set_requires_grad(module, flag):
    for p_ in module.parameters():
        p_.requires_grad_(flag)


def gan_iteration(netG, netD, optimizerG, optimizerD, imgs, sent_embs, words_embs, mask, noise, it_state,
                  opts=None):
    """One pass of the reference loop body (train_gan.py:185-291) on device tensors: the generated image, then `_d_step`, `_gp_step` and
    `_g_step`, which share an `_Iteration`.

    Returns a dict of 0-d loss tensors (no host sync).  ``it_state['i']`` carries the N_CRITIC counter.
    """
    opts = opts or StepOptions()
    batch_size = mask.size(0)
    ops.new_iteration(imgs.device)                 # one memset for all weight-gradient scratch of this iteration
    see = _DInput(netD, opts.diffaug, batch_size)
    psent_embs = sent_embs if cfg.DISC.SEPERATE else netG.proj_sent(sent_embs.float())
    nhwc_g = bool(getattr(netG, 'nhwc_out', False))             # generator can hand out its image in the engine layout
    # The discriminator does not couple the samples of a batch, so its passes over the real and the generated images
    # (193, 202) run as ONE pass over 2B images and the three COND_DNET calls (194, 203, 208) as one over 3B-1 rows: same
    # values, half the launches, twice the work per launch on the small maps at the end of D.  Not with spectral norm: there
    # every forward CALL advances the power iteration (modules.py:16-17), so the call pattern is part of the result.
    batched = nhwc_g and isinstance(netD, DF_DISC) and not cfg.DISC.SPEC_NORM and ops.fused_blocks() and not ops.debug_switch('no_d2b')
    # the discriminator's 2B-image input of the batched pass: the real images are converted into its first half, the
    # generator's last convolution writes its second half (no concatenation pass)
    both_h = (torch.empty((2 * batch_size, imgs.shape[2], imgs.shape[3], 8), dtype=ops.act_dtype(), device=imgs.device)
              if batched and getattr(netG, 'nhwc_dst_ok', False) else None)
    if nhwc_g:
        kw = dict(nhwc_dst=both_h[batch_size:]) if both_h is not None else {}
        fake, fake_h = netG(noise=noise, sent_embs=sent_embs, words_embs=words_embs, mask=mask, return_nhwc=True, **kw)
        assert both_h is None or fake_h.data_ptr() == both_h[batch_size:].data_ptr(), "generator ignored nhwc_dst"
    else:
        fake, fake_h = netG(noise=noise, sent_embs=sent_embs, words_embs=words_embs, mask=mask), None
    # converted once, used by both steps
    imgs_h = ops.to_nhwc8(imgs, out=both_h[:batch_size] if both_h is not None else None) if see.engine else None
    # data parallel: the trunk is handed out where it enters D's last blocks, for the two-part backward of the D step (parallel.py)
    cuts = [] if (parallel.active() and isinstance(netD, DF_DISC) and netD.cut_block() is not None
                  and not ops.debug_switch('no_dp_overlap')) else None
    it = _Iteration(netG=netG, netD=netD, optimizerG=optimizerG, optimizerD=optimizerD, opts=opts, see=see, batch_size=batch_size,
                    imgs=imgs, imgs_h=imgs_h, fake=fake, fake_h=fake_h, both_h=both_h, batched=batched, cuts=cuts,
                    sent_embs=sent_embs, psent_embs=psent_embs, labels=None, out={},
                    gather=parallel.gather_rows if opts.gather_negatives else (lambda t: t),
                    gather_all=parallel.gather_rows_multi if opts.gather_negatives else (lambda ts: list(ts)))   # several tensors, one collective
    _d_step(it)
    if cfg.TRAIN.MAGP:
        _gp_step(it)
    it_state['i'] = it_state.get('i', 0) + 1
    if it_state['i'] % cfg.TRAIN.N_CRITIC == 0:
        _g_step(it)
        it_state['i'] = 0
    it.out['fake'] = fake.detach()
    ops.end_iteration(imgs.device)                 # forward-only code between iterations (evaluation, sampling) stays out of the arena
    return it.out


class _DInput:
    """How ``netD`` sees an image; built once per iteration.  The one place that knows the engine layout's entrance (``nhwc8=``), the
    conversions and the augmentation (opts.diffaug; not in the reference): with it EVERY image netD sees goes through ops.diffaug first,
    with the rows of the sampler's static device tensor that belong to the pass, while `out['fake']`, the sample grids and eval() keep the
    plain images."""

    def __init__(self, netD, aug, batch_size):
        if aug is not None and aug.batch != batch_size:
            raise ValueError(f'DiffAugment was built for batches of {aug.batch}, got {batch_size}')
        self.netD, self.aug = netD, aug
        self.engine = isinstance(netD, DF_DISC)         # (a discriminator of another class has no engine-layout entrance)

    def rows(self, which):
        """the augmentation rows of the pass 'd' (2B), 'real', 'fake' or 'g'; None without augmentation"""
        return None if self.aug is None else getattr(self.aug, 'rows_' + which)()

    def __call__(self, x, x_h, rows):
        """netD's features of the images ``x`` (NCHW; may be None when ``x_h`` is given), ``x_h`` the same in the engine layout [B,H,W,8] or
        None, augmented with ``rows`` unless None.  What NetD.forward infers from its arguments stays with it (df_gan.py:145-150)."""
        netD = self.netD
        if not self.engine:
            return netD(x) if rows is None else netD(ops.to_nchw(self.aug(ops.to_nhwc8(x), rows), x.shape[1]))
        if rows is None:
            return netD(x, nhwc8=x_h) if x_h is not None else netD(x)
        return netD(None, nhwc8=self.aug(x_h if x_h is not None else ops.to_nhwc8(x), rows))


class _Iteration(types.SimpleNamespace):
    """What the phases of one iteration share: the modules, optimizers and ``opts``; the batch (``imgs``, ``imgs_h`` its engine layout or
    None, ``sent_embs``, ``psent_embs``) and the generated images (``fake``, ``fake_h``); ``see`` (the `_DInput`), ``batched`` with its input
    buffer ``both_h``, ``cuts``, the gather functions; ``labels``, which the D step leaves for the G step; ``out``, the returned losses."""


def _scaled(loss, scaler):
    """IEEE-half mode only (ops.set_precision): each backward runs on a dynamic, device-resident scale x its loss (keeps 1/B-sized
    gradients normal), HipAdam reads the f32 parameter gradients times 1 / scale and SKIPS the step on the device when one
    of them is inf / NaN (after the all-reduce, so every rank decides alike).  ``scaler`` is None in the other modes."""
    return scaler.scale(loss) if scaler is not None else loss


def _backward_in_two_parts(loss, netD, cuts):
    """D's head and last three blocks hold 93 % of its gradient bytes (75 of 81 MB at 256 px) and their backward is the first quarter of
    the pass (small maps); the blocks before the cut hold 7 % and take the rest of the time (large maps).  The first part's all-reduce is
    started as soon as its gradients exist and runs beside the second part; same gradients as one `.backward()` (autograd executes the
    same nodes in the same order, in two calls)."""
    late, early = netD.late_parameters()
    late = [p_ for p_ in late if p_.requires_grad]
    gs = torch.autograd.grad(loss, cuts + late, allow_unused=True)
    for p_, g_ in zip(late, gs[len(cuts):]):
        p_.grad = g_
    pending = parallel.allreduce_mean_grads_begin(late)
    reached = [(c_, g_) for c_, g_ in zip(cuts, gs) if g_ is not None]          # (a handed-out tensor the loss does not use has no gradient)
    torch.autograd.backward([c_ for c_, _ in reached], [g_ for _, g_ in reached])
    parallel.allreduce_mean_grads_end(pending, early)


def _d_step(it):
    """the discriminator step (train_gan.py:187-229)"""
    T, E, netD, see, B, out = cfg.TRAIN, cfg.TRAIN.ENCODER_LOSS, it.netD, it.see, it.batch_size, it.out
    ps_d = it.psent_embs.detach()
    fake_hd = it.fake_h.detach() if it.fake_h is not None else None
    netD.cut_sink = it.cuts
    # the two forms differ in how they come by (outputs_real, logits_real, logits_fake, logits_mismatch or None)
    if it.batched:      # one pass over 2B images, one COND_DNET call over 3B-1 rows
        x2b = it.both_h if it.both_h is not None else torch.cat((it.imgs_h, fake_hd))
        feats = see(None, x2b, see.rows('d'))
        real_features = feats[:B]
        rows = [feats, real_features[:B - 1]] if T.RMIS_LOSS else [feats]
        sents = [ps_d, ps_d, ps_d[1:B]] if T.RMIS_LOSS else [ps_d, ps_d]
        o_all = netD.COND_DNET(torch.cat(rows) if T.RMIS_LOSS else feats, sent_embs=torch.cat(sents))
        outputs_real = [o[:B] for o in o_all]
        logits_real, logits_fake = o_all[0][:B], o_all[0][B:2 * B]
        logits_mismatch = o_all[0][2 * B:] if T.RMIS_LOSS else None
    else:               # the reference's calls, one by one (193-194, 202-203, 208)
        real_features = see(it.imgs, it.imgs_h, see.rows('real'))
        outputs_real = netD.COND_DNET(real_features, sent_embs=ps_d)
        fake_features = see(it.fake.detach(), fake_hd, see.rows('fake'))
        logits_real, logits_fake = outputs_real[0], netD.COND_DNET(fake_features, sent_embs=ps_d)[0]
        logits_mismatch = netD.COND_DNET(real_features[:B - 1], sent_embs=it.psent_embs[1:B].detach())[0] if T.RMIS_LOSS else None
    netD.cut_sink = None
    errD_real = ops.hinge(logits_real, -1.0)
    errD_fake = ops.hinge(logits_fake, 1.0)
    mis_loss = errD_fake
    if T.RMIS_LOSS:
        errD_mismatch = ops.hinge(logits_mismatch, 1.0)
        mis_loss = mis_loss + errD_mismatch
        out['errD_mismatch'] = errD_mismatch.detach()
    n_rows = B * (parallel.world() if it.opts.gather_negatives else 1)
    enc_loss = 0.
    if E.SENT:
        assert cfg.DISC.SENT_MATCH or cfg.DISC.IMG_MATCH
        # (the sentence embeddings the labels are made from travel with the two embeddings the loss compares: one collective)
        g_sent, g_img, g_txt = it.gather_all((it.sent_embs.float(), outputs_real[1], outputs_real[2]))
        it.labels = make_labels(n_rows, sent_embs=g_sent, b_global=E.B_GLOBAL)
        ds_loss = sent_loss(imgs=g_img, txts=g_txt, labels=it.labels, b_global=E.B_GLOBAL)
        enc_loss = enc_loss + T.SMOOTH.SENT * ds_loss
        out['ds_loss'] = ds_loss.detach()
    elif E.WORD or E.DISC or E.VGG:
        it.labels = make_labels(n_rows, sent_embs=it.gather(it.sent_embs.float()), b_global=E.B_GLOBAL)
    if E.WORD:
        raise NotImplementedError
    errD = errD_real + (mis_loss * T.SMOOTH.MISMATCH) + enc_loss
    it.netG.zero_grad()
    netD.zero_grad()
    sc_d = ops.loss_scaler("D", it.imgs.device)
    if it.cuts:
        _backward_in_two_parts(_scaled(errD, sc_d), netD, it.cuts)
    else:
        _scaled(errD, sc_d).backward()
        parallel.allreduce_mean_grads(netD.parameters())
    _step(it.optimizerD, sc_d)
    out.update(errD=errD.detach(), errD_real=errD_real.detach(), errD_fake=errD_fake.detach())


def _gp_step(it):
    """the matching-aware gradient penalty on real pairs (train_gan.py:231-252)"""
    netD, see = it.netD, it.see
    interpolated = it.imgs.detach().requires_grad_()
    sent_inter = it.psent_embs.detach().requires_grad_()
    # this forward's backward is differentiated again.  The fused discriminator blocks carry their own second-order node
    # (ops.ResDBwdFn); with spectral norm the blocks are composed from the fine-grained Functions as before
    # ops.second_order(): the blocks keep their residual branch (not just its sign bits) for the linearised forward
    with (ops.composable() if cfg.DISC.SPEC_NORM else contextlib.nullcontext()), ops.second_order():
        # (the leaf itself goes in as x.  Augmented: the penalty is taken where the discriminator is evaluated, and differentiated
        # through the augmentation)
        features = see(interpolated, None, see.rows('real'))
        o = netD.COND_DNET(features, sent_inter)
    s_in = ops.gp_inner_scale()    # IEEE-half mode: the inner backward runs on s_in x ones, the penalty divides it out
    with ops.no_wgrad():           # first-order pass only needs d(logit)/d(inputs)
        grads = torch.autograd.grad(outputs=o[0], inputs=(interpolated, sent_inter),
                                    grad_outputs=torch.full_like(o[0], s_in), retain_graph=True, create_graph=True,
                                    only_inputs=True)
    # mean(||cat(grad0, grad1)||_2 ** 6) (241-247) in two passes over the 3*S*S-wide image gradient, no concatenation
    d_loss_gp = ops.grad_penalty(grads[0], grads[1], inner_scale=s_in)
    d_loss = 2.0 * d_loss_gp
    it.optimizerD.zero_grad()
    it.optimizerG.zero_grad()
    sc_gp = ops.loss_scaler("GP", it.imgs.device)
    _scaled(d_loss, sc_gp).backward()
    # the reference's autograd hands zero (not None) grads to every bias that feeds the logit
    # (their only path is through LeakyReLU'' == 0), which still advances Adam's moments/step.
    for name, p_ in netD.named_parameters():
        if p_.grad is None and name.endswith('.bias') and 'proj_match' not in name and _bias_on_logit_path(netD, name):
            p_.grad = torch.zeros_like(p_)
    parallel.allreduce_mean_grads(netD.parameters())
    _step(it.optimizerD, sc_gp)
    it.out['d_loss_gp'] = d_loss_gp.detach()


def _bias_on_logit_path(netD, name):
    """conv_img.bias and the conv_s.bias of blocks whose learned shortcut is active (df_gan.py:286-288)."""
    if name == 'conv_img.bias':
        return True
    if name.startswith('downblocks.') and name.endswith('.conv_s.bias'):
        return netD.downblocks[int(name.split('.')[1])].learned_shortcut
    return False


def _g_step(it):
    """the generator step (train_gan.py:254-291)"""
    T, E, netD, see, out = cfg.TRAIN, cfg.TRAIN.ENCODER_LOSS, it.netD, it.see, it.out
    _set_requires_grad(netD, False)          # D's weight grads would be discarded (zero_grad at 226-227)
    try:
        features = see(it.fake, it.fake_h, see.rows('g'))
        outputs = netD.COND_DNET(features, sent_embs=it.psent_embs)
        errG_fake = -outputs[0].float().mean()
        enc_loss = 0.0
        real_pooled = fake_pooled = real_vgg = fake_vgg = None
        if E.VGG:
            if it.opts.vgg is None:
                raise ImportError('TRAIN.ENCODER_LOSS.VGG is on and the iteration was handed no VGG-19: --vgg_weights PATH (StepOptions(vgg=))')
            # the plain images, not the augmented ones: the augmentation is there for the discriminator's overfitting, and VGG is not it
            real_vgg, fake_vgg = it.opts.vgg.rows(it.imgs_h if it.imgs_h is not None else ops.to_nhwc8(it.imgs),
                                                  it.fake_h if it.fake_h is not None else ops.to_nhwc8(it.fake))
        if E.DISC:
            with torch.no_grad():            # (augmented: the same rows as the generated images it is compared with)
                real_pooled = ops.global_avgpool(see(it.imgs, it.imgs_h, see.rows('g')).permute(0, 2, 3, 1).contiguous())
            fake_pooled = ops.global_avgpool(features.permute(0, 2, 3, 1).contiguous())
        # what the contrastive terms of this step compare across ranks, all-gathered in ONE collective (a seam of the captured iteration each)
        rows = it.gather_all(([outputs[1], outputs[2]] if E.SENT else []) + ([real_pooled, fake_pooled] if E.DISC else [])
                             + ([real_vgg, fake_vgg] if E.VGG else []))
        if E.SENT:
            gs_loss = sent_loss(imgs=rows[0], txts=rows[1], labels=it.labels, b_global=E.B_GLOBAL)
            enc_loss = enc_loss + T.SMOOTH.SENT * gs_loss
            out['gs_loss'] = gs_loss.detach()
        if E.WORD:
            raise NotImplementedError
        if E.DISC:
            d0 = 2 if E.SENT else 0
            disc_loss = img_loss(real_imgs=rows[d0], fake_imgs=rows[d0 + 1], labels=it.labels, b_global=E.B_GLOBAL)
            enc_loss = enc_loss + T.SMOOTH.DISC * disc_loss
            out['disc_loss'] = disc_loss.detach()
        if E.VGG:
            vgg_loss = img_loss(real_imgs=rows[-2], fake_imgs=rows[-1], labels=it.labels, b_global=E.B_GLOBAL)
            enc_loss = enc_loss + it.opts.vgg_smooth * vgg_loss
            out['vgg_loss'] = vgg_loss.detach()
        errG = errG_fake + enc_loss
        it.netG.zero_grad()
        netD.zero_grad()
        sc_g = ops.loss_scaler("G", it.imgs.device)
        _scaled(errG, sc_g).backward()
    finally:
        _set_requires_grad(netD, True)
    parallel.allreduce_mean_grads(it.netG.parameters())
    _step(it.optimizerG, sc_g, it.opts.ema)
    out.update(errG=errG.detach(), errG_fake=errG_fake.detach())


# --------------------------------------------------------------------------------------- synthetic front end
class SyntheticCOCO:
    """COCO-shaped random batches with the tuple layout of the reference loader ``(imgs, [(caps, cap_lens)], keys)``
    (dataset.py:64): images uniform in [-1,1] like Normalize(0.5,0.5) output (dataset.py:34-37), captions as WordTextDataset
    pads them (int64 token ids in [1, V), zeros after the length; dataset.py:104-111)."""

    def __init__(self, n_batches, batch_size, img_size, max_len, seed, voca_size=27297, distinct=4):
        """``distinct``: batches i and i + distinct are the same tensors (all generated before the first one is handed out and kept in
        pinned host memory): drawing 50 M uniform numbers per 256 x 256 x 256 batch takes the host ~0.25 s, six times the iteration
        it feeds."""
        self.n, self.bs, self.size, self.max_len, self.seed, self.voca = n_batches, batch_size, img_size, max_len, seed, voca_size
        self.distinct = max(1, min(int(distinct), n_batches))
        self._cache = {}

    def __len__(self):
        return self.n

    def _batch(self, i):
        if i not in self._cache:
            g = torch.Generator().manual_seed(self.seed * 100003 + i)
            imgs = torch.rand(self.bs, 3, self.size, self.size, generator=g) * 2 - 1
            if torch.cuda.is_available():
                imgs = imgs.pin_memory()
            lens = torch.randint(5, self.max_len + 1, (self.bs,), generator=g)
            caps = torch.randint(1, self.voca, (self.bs, self.max_len), generator=g)
            caps = caps * (torch.arange(self.max_len)[None, :] < lens[:, None])
            self._cache[i] = (imgs, caps, lens)
        return self._cache[i]

    def __iter__(self):
        for i in range(self.distinct):
            self._batch(i)
        for i in range(self.n):
            imgs, caps, lens = self._batch(i % self.distinct)
            yield imgs, [(caps, lens)], [f'syn{i}_{j}' for j in range(self.bs)]


class SyntheticTextEncoder(torch.nn.Module):
    """Stands in for the frozen SBERT encoder (encoder.py:24-70; third-party package + checkpoint): returns
    words_embs [B,E,T], sent_embs [B,E], mask [B,T] (True = padding) as random tensors that are a function of the captions."""

    def __init__(self, emb_dim, max_len, seed, device):
        super().__init__()
        self.e, self.t, self.seed, self.device = emb_dim, max_len, seed, device

    def forward(self, caps, cap_lens):
        caps = torch.as_tensor(caps).cpu()
        g = torch.Generator().manual_seed(self.seed * 7919 + int(caps[0, :4].sum()))
        B = cap_lens.size(0)
        words = torch.randn(B, self.e, self.t, generator=g)
        sent = torch.randn(B, self.e, generator=g)
        mask = torch.arange(self.t)[None, :] >= cap_lens.cpu()[:, None]
        return words.to(self.device), sent.to(self.device), mask.to(self.device)


# --------------------------------------------------------------------------------------- epoch loop
_TIMED_FROM = 4          # train() reports images/s from the end of this step on: two eager warm-ups, the capture(s), one replay
def _log_epoch_scalars(writer, last, epoch):
    """the per-epoch scalars of the reference (train_gan.py:300-320): the losses of the epoch's last iteration"""
    if writer is None or 'errD' not in last:
        return
    writer.add_scalar('epoch', epoch, epoch)
    for tag, key in (('Loss_D', 'errD'), ('Loss_G', 'errG'), ('errD_real', 'errD_real'), ('errD_fake', 'errD_fake'),
                     ('errD_mismatch', 'errD_mismatch'), ('ds_loss', 'ds_loss'), ('gs_loss', 'gs_loss'), ('disc_loss', 'disc_loss'),
                     ('vgg_loss', 'vgg_loss')):
        if key in last:
            writer.add_scalar(tag, last[key].item(), epoch)
    writer.flush()


class _DeviceBatches:
    """The loader's batches with the image tensor already on its way to the device: while iteration i runs (a graph replay leaves the
    host idle), batch i+1 is fetched and uploaded on a side stream from pinned memory, so the 0.2 GB of a 256 x 256 x 256 f32 batch
    (~5 ms of PCIe time) is off the iteration's critical path.  Yields the loader's tuples with `imgs` on the device."""

    def __init__(self, loader, device):
        self.loader, self.device = loader, device
        self.stream = torch.cuda.Stream(device=device) if device.type == 'cuda' else None

    def __len__(self):
        return len(self.loader)

    def _upload(self, data):
        imgs, texts_lst, keys = data
        if self.stream is None or not torch.is_tensor(imgs) or imgs.is_cuda:
            return (imgs.to(self.device) if torch.is_tensor(imgs) else imgs, texts_lst, keys), imgs, None
        host = imgs if imgs.is_pinned() else imgs.pin_memory()
        with torch.cuda.stream(self.stream):
            dev = host.to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        return (dev, texts_lst, keys), host, ev

    def __iter__(self):
        it = iter(self.loader)
        try:
            nxt = self._upload(next(it))
        except StopIteration:
            return
        while nxt is not None:
            (dev, texts_lst, keys), host, ev = nxt
            if ev is not None:
                torch.cuda.current_stream().wait_event(ev)
                dev.record_stream(torch.cuda.current_stream())
            yield dev, texts_lst, keys, host
            try:                       # (after the consumer has launched its iteration: this upload overlaps it)
                nxt = self._upload(next(it))
            except StopIteration:
                nxt = None


def encode(text_encoder, caps, cap_lens, keys):
    """(words_embs, sent_embs, mask) of a batch: a CachedTextEncoder looks it up by its keys, an encoder encodes the captions"""
    return text_encoder.forward_keys(keys) if hasattr(text_encoder, 'forward_keys') else text_encoder(caps, cap_lens)


def _log_first_batch(img_dir, train_loader, caps, cap_lens, imgs_host, sent_embs, words_embs, mask, device):
    """``sents.txt`` and ``imgs.png`` of the first batch (train_gan.py:146-160); returns the fixed noise and captions of the per-epoch grids"""
    i2w = getattr(getattr(train_loader, 'dataset', None), 'i2w', None)
    with open(f'{img_dir}/sents.txt', 'w') as f:
        if torch.is_tensor(caps):            # WORD captions: token ids (index_to_sent, dataset.py) or the ids themselves
            for row, n in zip(caps.tolist(), torch.as_tensor(cap_lens).tolist()):
                f.write((' '.join(i2w[t] for t in row[:n]) if i2w else ' '.join(str(t) for t in row[:n])) + ' \n')
        else:                                # SENT captions: the sentences
            for sent in caps:
                f.write(f'{sent} \n')
    fixed = dict(noise=torch.randn(mask.size(0), cfg.TRAIN.NOISE_DIM).to(device), sent=sent_embs.clone(),
                 words=words_embs.clone(), mask=mask.clone())
    save_image(imgs_host, f'{img_dir}/imgs.png', normalize=True, scale_each=True)
    return fixed


def _graphed_iteration(step_fn, inputs):
    return GraphedIteration(step_fn, inputs, n_critic=cfg.TRAIN.N_CRITIC, warmup=2)


class IterationRunner:
    """Runs a batch as hipGraph replays (``use_graph``; the graphed object is made from the first batch by ``factory``) or with eager
    launches: ``--graph 0``, a batch of another shape than the captured one (a loader without drop_last), and every batch after a capture
    that failed in a single process.  Nothing else is caught: a warm-up iteration or a replay that raises may already have applied an
    optimizer step, so running that batch again would step twice.  Owns the N_CRITIC counter ``it_state``."""

    def __init__(self, step_fn, logger, use_graph, factory=_graphed_iteration):
        self.step_fn, self.logger, self.use_graph, self.factory = step_fn, logger, use_graph, factory
        self.it_state, self.graphed = {}, None

    @property
    def hipgraph(self):
        return self.graphed is not None

    def __call__(self, inputs):
        if self.use_graph and self.graphed is None:
            self.graphed = self.factory(self.step_fn, inputs)
            self.graphed.it_state = self.it_state
        if self.graphed is not None and all(s_.shape == t_.shape and s_.dtype == t_.dtype for s_, t_ in zip(self.graphed.static_in, inputs)):
            try:
                return dict(self.graphed(*inputs))
            except CaptureFailed as e:       # (an operator that synchronises, memory): nothing the capture recorded has run
                if parallel.world() > 1:
                    raise                    # the ranks' collectives are out of step: no in-band way to agree on a fallback
                self.logger.info(f'hipGraph capture failed ({e}); continuing with eager launches')
                self.it_state = dict(self.graphed.it_state)
                self.close()
                self.use_graph = False
        return self.step_fn(*inputs, self.it_state)

    def close(self):
        if self.graphed is not None:
            self.graphed.close()
            self.graphed = None


class _Throughput:
    """The run's images/s: from the end of step _TIMED_FROM (warm-ups and captures done) to the end of each epoch, one synchronisation
    per epoch.  ``last`` is the latest report, the ``throughput`` entry of what train() returns."""

    def __init__(self, device, logger):
        self.device, self.logger, self.t0, self.n0, self.last = device, logger, None, 0, None

    def after_step(self, nsteps):
        if self.device.type == 'cuda' and self.t0 is None and nsteps == _TIMED_FROM + 2 * (cfg.TRAIN.N_CRITIC - 1):
            torch.cuda.synchronize(self.device)
            self.t0, self.n0 = time.perf_counter(), nsteps + 1

    def after_epoch(self, nsteps, hipgraph):
        if self.t0 is None or nsteps <= self.n0:
            return
        torch.cuda.synchronize(self.device)
        dt_, n_ = time.perf_counter() - self.t0, nsteps - self.n0
        thr = self.last = dict(steps=n_, seconds=round(dt_, 4), ms_per_step=round(1e3 * dt_ / n_, 3),
                               images_per_s=round(parallel.world() * cfg.TRAIN.BATCH_SIZE * n_ / dt_, 1), hipgraph=hipgraph)
        self.logger.info(f'throughput: {thr["images_per_s"]} images/s ({thr["ms_per_step"]} ms per iteration over {n_} iterations, '
                         f'{"hipGraph replay" if hipgraph else "eager launches"})')
        self.t0, self.n0 = time.perf_counter(), nsteps


_CHECKPOINT = dict(netG='netG_{:03d}.pth', netD='netD_{:03d}.pth', optimizerG='optimizerG.pth', optimizerD='optimizerD.pth',
                   loss_scale='loss_scale.pth', netG_ema='netG_ema_{:03d}.pth', ema_state='ema_state.pth')


def _ckpt(model_dir, what, epoch):
    return f'{model_dir}/{_CHECKPOINT[what].format(epoch)}'


def save_checkpoint(model_dir, epoch, netG, netD, optimizerG, optimizerD, ema=None, netG_ema=None):
    """The reference's four files (train_gan.py:328-334); ``loss_scale.pth`` where there is scaler state (IEEE-half mode: the dynamic loss
    scales are optimizer state too); with ``ema``, the averaged generator ``netG_ema`` as a plain generator state dict, loadable wherever
    ``netG_<epoch>.pth`` is, and the average's counter."""
    for what, obj in (('netG', netG), ('netD', netD), ('optimizerG', optimizerG), ('optimizerD', optimizerD)):
        torch.save(obj.state_dict(), _ckpt(model_dir, what, epoch))
    if ops.loss_scaler_state():
        torch.save(ops.loss_scaler_state(), _ckpt(model_dir, 'loss_scale', epoch))
    if ema is not None:
        torch.save(netG_ema.state_dict(), _ckpt(model_dir, 'netG_ema', epoch))
        torch.save(dict(num_updates=int(ema.num_updates.item()), decay=ema.decay, start=ema.start), _ckpt(model_dir, 'ema_state', epoch))


def load_checkpoint(model_dir, epoch, netG, netD, optimizerG, optimizerD, ema=None, *, device, logger):
    """`save_checkpoint`'s files of ``epoch`` back into the objects; ``ema`` (a `ParamEMA` of the loaded ``netG``): `load_average` too"""
    for what, obj in (('netG', netG), ('netD', netD), ('optimizerG', optimizerG), ('optimizerD', optimizerD)):
        obj.load_state_dict(torch.load(_ckpt(model_dir, what, epoch), map_location=device))
    if os.path.isfile(_ckpt(model_dir, 'loss_scale', epoch)):
        ops.load_loss_scaler_state(torch.load(_ckpt(model_dir, 'loss_scale', epoch), map_location='cpu'), device)
    logger.info(f'Load models, epoch : {epoch}')
    if ema is not None:
        load_average(model_dir, epoch, ema, device, logger)


def load_average(model_dir, epoch, ema, device, logger):
    """the average's two files into ``ema``, which was built from the resumed generator: without them (a checkpoint written without the
    average) it stays a copy of those weights"""
    f_w, f_s = _ckpt(model_dir, 'netG_ema', epoch), _ckpt(model_dir, 'ema_state', epoch)
    if not (os.path.isfile(f_w) and os.path.isfile(f_s)):
        return logger.info(f'no {os.path.basename(f_w)} / {os.path.basename(f_s)} in {model_dir}: the EMA starts from '
                           f'{os.path.basename(_ckpt(model_dir, "netG", epoch))}')
    saved = torch.load(f_s, map_location='cpu')
    ema.load_state_dict(dict(shadow=torch.load(f_w, map_location=device), num_updates=saved['num_updates']))
    logger.info(f'Load EMA generator, epoch : {epoch} ({saved["num_updates"]} updates; saved with decay {saved["decay"]}, start {saved["start"]})')


def _end_of_epoch(epoch, last, *, netG, netD, optimizerG, optimizerD, ema, netG_ema, fixed, img_dir, model_dir, test_loader, text_encoder,
                  logger, writer, eval_opts, clip_dir=None, clip_max_tokens=64):
    """what the reference does after an epoch's last batch (train_gan.py:300-336): scalars, the sample grid from the fixed batch, and past
    epoch 50 the checkpoint and `eval`; with ``ema`` the grid, the checkpoint and `eval` take the averaged generator"""
    if parallel.rank() == 0:
        _log_epoch_scalars(writer, last, epoch)
    # IEEE-half mode: the dynamic loss scales and the optimizer steps the found-inf check skipped so far (one host read per epoch)
    sc_stats = ops.loss_scaler_stats()
    if sc_stats:
        last['loss_scale'] = sc_stats
        logger.info('loss scale ' + ' '.join(f"{k}: {v['scale']:g} ({v['skipped_steps']} skipped)" for k, v in sc_stats.items()))
        if all(v['scale'] <= 1.0 and v['last_step_skipped'] for v in sc_stats.values()):
            raise FloatingPointError('every backward of the f16 mode overflows at loss scale 1: the run has diverged')
    if ema is not None and parallel.rank() == 0:
        ema.copy_to(netG_ema)                # this epoch's averaged generator (grid, checkpoint, eval)
    gen = netG_ema if ema is not None else netG
    if fixed is not None:
        with torch.no_grad():
            gen.eval()
            fake = gen(noise=fixed['noise'], sent_embs=fixed['sent'], words_embs=fixed['words'], mask=fixed['mask'])
            save_image_async(fake, f'{img_dir}/fake_samples_epoch_{epoch:03d}.png', normalize=True, scale_each=True)
    if epoch > 50 and parallel.rank() == 0:
        save_checkpoint(model_dir, epoch, netG, netD, optimizerG, optimizerD, ema, netG_ema)
        logger.info('Save models')
        if test_loader is not None:
            # (--caption_cache: the test split's rows are another table; the train split's encoder carries the test split's)
            eval(loader=test_loader, state_epoch=epoch, text_encoder=getattr(text_encoder, 'eval_encoder', None) or text_encoder, netG=gen,
                 logger=logger, num_samples=6000, save_dir=f'{img_dir}/test' if img_dir else None, org_dir=f'{img_dir}/org' if img_dir else None,
                 writer=writer, eval_opts=eval_opts, clip_dir=clip_dir, **_clip_tokens_arg(clip_max_tokens))


def train(train_loader, test_loader, state_epoch, text_encoder, netG, netD, optimizerG, optimizerD, logger, model_dir,
          opts=None, img_dir=None, max_steps=None, writer=None, eval_opts=None, clip_dir=None, clip_max_tokens=64):
    """Epoch loop with the reference's signature (train_gan.py:142); returns the last iteration's losses.

    With ``img_dir`` (rank 0) it keeps the reference's visual log: ``sents.txt`` and ``imgs.png`` of the first batch (146-160),
    ``fake_samples_<step>.png`` every LOG_INTERVAL steps (298-299), ``fake_samples_epoch_<epoch>.png`` from a fixed noise /
    caption batch in eval mode after every epoch (322-326); with ``writer`` the per-epoch scalars (300-320).

    ``opts.graph`` (the entry point's default, ``--graph 1``): the loop body runs as hipGraph replays
    (xmc_gan_amd.graph.GraphedIteration: two eager warm-up iterations, one capture per N_CRITIC phase, collectives as eager
    seams between graph segments); a batch is copied into the graph's static inputs and the losses stay on the device until they
    are logged -- at the first step and every LOG_INTERVAL steps unless ``opts.log_each_step``.

    ``opts.ema`` (a `ParamEMA` of ``netG``, ``--ema_decay``): the per-epoch grid and `eval` sample from the averaged weights,
    written into a second, eval-mode generator that exists for nothing else (the captured iteration never sees it); checkpoints
    add ``netG_ema_<epoch>.pth`` (a plain generator state dict) and ``ema_state.pth``.  ``netG`` itself keeps training.

    ``opts.diffaug`` (a `DiffAugment`, ``--diffaug``): its rows are redrawn before every iteration, graphed or eager.
    ``eval_opts`` (an `EvalOptions`) and ``clip_dir`` (CLIPScore's model directory): what `eval` scores after an epoch, handed on to it,
    as is ``clip_max_tokens`` (`CLIPScorer`'s ``max_tokens``)."""
    device = next(netG.parameters()).device
    opts = opts or StepOptions()
    ema = opts.ema
    netG_ema = type(netG)(cfg).to(device).eval().requires_grad_(False) if ema is not None else None
    last, nsteps, fixed = {}, 0, None
    visual = img_dir is not None and parallel.rank() == 0
    batches = _DeviceBatches(train_loader, device)
    clock = _Throughput(device, logger)
    runner = IterationRunner(lambda *inputs_and_state: gan_iteration(netG, netD, optimizerG, optimizerD, *inputs_and_state, opts),
                             logger, use_graph=bool(opts.graph) and device.type == 'cuda')

    def finish():            # the one way out: the sample grids queued for the writer thread are on disk when train() returns
        flush_saves()
        out = _detached(last)
        if clock.last is not None:
            out['throughput'] = clock.last
        if runner.hipgraph:
            out['hipgraph'] = True
        runner.close()
        return out

    for epoch in range(state_epoch + 1, cfg.TRAIN.MAX_EPOCH + 1):
        netG.train()
        netD.train()
        sampler = getattr(train_loader, 'sampler', None)
        if isinstance(sampler, torch.utils.data.distributed.DistributedSampler):
            sampler.set_epoch(epoch)             # data parallel: a new permutation (and new per-rank shards) every epoch
        for step, (imgs, texts_lst, keys, imgs_host) in enumerate(batches):
            caps, cap_lens = texts_lst[0]
            with torch.no_grad():
                words_embs, sent_embs, mask = encode(text_encoder, caps, cap_lens, keys)
            words_embs, sent_embs = words_embs.detach(), sent_embs.detach()
            if visual and fixed is None:         # the reference takes these from the loader's first batch before the loop
                fixed = _log_first_batch(img_dir, train_loader, caps, cap_lens, imgs_host, sent_embs, words_embs, mask, device)
            noise = torch.randn(mask.size(0), cfg.TRAIN.NOISE_DIM).to(device, non_blocking=True)   # CPU generator, as upstream (197-198)
            if opts.diffaug is not None:         # new augmentation rows, outside any capture: the replayed kernels read them from the device
                opts.diffaug.refresh()
            last = runner((imgs, sent_embs, words_embs, mask, noise))
            clock.after_step(nsteps)
            if 'errG' in last and (opts.log_each_step or nsteps == 0 or (step + 1) % cfg.TRAIN.LOG_INTERVAL == 0):
                logger.info(f'[{epoch}/{cfg.TRAIN.MAX_EPOCH}][{step + 1}/{len(train_loader)}] '
                            f'Loss_D: {last["errD"].item():.3f} Loss_G: {last["errG"].item():.3f} '
                            f'errD_real: {last["errD_real"].item():.3f} errD_fake: {last["errD_fake"].item():.3f} ')
            if visual and (step + 1) % cfg.TRAIN.LOG_INTERVAL == 0:
                # (copied to the host now, encoded on the writer thread: utils/visual.py)
                save_image_async(last['fake'], f'{img_dir}/fake_samples_{step + 1:03d}.png', normalize=True, scale_each=True)
            nsteps += 1
            if max_steps is not None and nsteps >= max_steps:
                return finish()
        clock.after_epoch(nsteps, runner.hipgraph)
        _end_of_epoch(epoch, last, netG=netG, netD=netD, optimizerG=optimizerG, optimizerD=optimizerD, ema=ema, netG_ema=netG_ema,
                      fixed=fixed, img_dir=img_dir, model_dir=model_dir, test_loader=test_loader, text_encoder=text_encoder,
                      logger=logger, writer=writer, eval_opts=eval_opts, clip_dir=clip_dir, clip_max_tokens=clip_max_tokens)
    return finish()


def _detached(last):
    """the last iteration's losses as tensors of their own (a graph's static outputs are overwritten by the next replay and freed with it)"""
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in last.items()}


# what `eval` scores after an epoch (not part of the reference cfg; main() fills one from --fid_inception, --prdc and --damsm_image_encoder)
EvalOptions = collections.namedtuple('EvalOptions', 'fid_inception prdc_k damsm_image_encoder kid kid_subsets kid_subset_size inception_score',
                                     defaults=('', 0, '', False, 100, 1000, 0))


_EVAL_REPORT = {    # metric of MetricSuite.results(): (its log line, the values that are scalars of that name, the line that says why there is none)
    'FID': (' epoch {epoch}, FID : {FID}', ('FID',), ' epoch {epoch}, generated {cnt} images (FID not computed: {why})'),
    'PRDC': (' epoch {epoch}, precision : {precision} recall : {recall} density : {density} coverage : {coverage} (k={k}, n={n_real}/{n_fake})',
             ('precision', 'recall', 'density', 'coverage'), ' epoch {epoch}, precision / recall / density / coverage not computed: {why}'),
    'R-precision': (' epoch {epoch}, R-precision : {r_precision} +- {std} (k={k}, n={n})', ('r_precision',),
                    ' epoch {epoch}, R-precision not computed: {why}'),
    'KID': (' epoch {epoch}, KID : {kid} +- {std} (subsets={subsets}, size={subset_size}, n={n_real}/{n_fake})', ('kid',),
            ' epoch {epoch}, KID not computed: {why}'),
    'IS': (' epoch {epoch}, IS : {inception_score} +- {std} (splits={splits}, n={n})', ('inception_score',),
           ' epoch {epoch}, IS not computed: {why}'),
    'CLIPScore': (' epoch {epoch}, CLIPScore : {clip_score} +- {std} (n={n}, model={model})', ('clip_score',),
                  ' epoch {epoch}, CLIPScore not computed: {why}'),
}
_EVAL_SCALAR = {'r_precision': 'R_precision', 'kid': 'KID', 'inception_score': 'IS', 'clip_score': 'CLIPScore'}     # a value's name -> its scalar's
_EVAL_METRICS_KEY = {('PRDC', 'k'): 'prdc_k', ('KID', 'std'): 'kid_std', ('KID', 'subsets'): 'kid_subsets', ('KID', 'subset_size'): 'kid_subset_size',
                     ('KID', 'n_real'): 'kid_n_real', ('KID', 'n_fake'): 'kid_n_fake',
                     ('IS', 'std'): 'inception_score_std', ('IS', 'splits'): 'inception_score_splits', ('IS', 'n'): 'inception_score_n',
                     ('CLIPScore', 'std'): 'clip_score_std', ('CLIPScore', 'cosine'): 'clip_score_cosine', ('CLIPScore', 'n'): 'clip_score_n',
                     ('CLIPScore', 'n_truncated'): 'clip_score_n_truncated', ('CLIPScore', 'model'): 'clip_score_model'}


def _caption_strings(caps, cap_lens, loader):
    """the caption strings of a batch for CLIPScore: SENT captions as they are, WORD captions through the dataset's ``i2w``; None where
    neither is there (--synthetic)"""
    if len(caps) and all(isinstance(c, str) for c in caps):
        return list(caps)
    i2w = getattr(getattr(loader, 'dataset', None), 'i2w', None)
    if not i2w or not torch.is_tensor(caps):
        return None
    return [' '.join(i2w[t] for t in row[:n]) for row, n in zip(caps.tolist(), torch.as_tensor(cap_lens).tolist())]


def _new_metric_args(given, kid, kid_subsets, kid_subset_size, inception_score):
    """the keyword arguments of `MetricSuite` for KID and the Inception Score: none at all while both are off"""
    kid = given.kid if kid is None else kid
    splits = given.inception_score if inception_score is None else inception_score
    kw = {}
    if kid:
        kw.update(kid=True, kid_subsets=given.kid_subsets if kid_subsets is None else kid_subsets,
                  kid_subset_size=given.kid_subset_size if kid_subset_size is None else kid_subset_size)
    if splits:
        kw.update(inception_score=int(splits))
    return kw


def _clip_tokens_arg(clip_max_tokens):
    """``clip_max_tokens`` as a keyword, and no argument at all at the default of 64"""
    return {} if int(clip_max_tokens) == 64 else {'clip_max_tokens': int(clip_max_tokens)}


@torch.no_grad()
def eval(loader, state_epoch, text_encoder, netG, logger, num_samples=6000, save_dir=None, org_dir=None, writer=None, fid_inception=None,
         damsm_image_encoder=None, metrics=None, prdc=None, eval_opts=None, kid=None, kid_subsets=None, kid_subset_size=None,
         inception_score=None, clip_dir=None, clip_max_tokens=64):
    """Generate images for the test loader and score them (train_gan.py:338-395): every generated image goes to ``save_dir/<key>.png`` and,
    unless ``org_dir`` already holds ``num_samples`` files, every real one to ``org_dir/<key>.png``, as 8-bit PNGs of (x + 1) * 127.5.  The
    scores are a `MetricSuite`'s (xmc_gan_amd/evaluate.py): FID with ``fid_inception`` (without it: between the two directories, when
    ``pytorch_fid`` imports), precision / recall / density / coverage with ``prdc`` = K > 0 beside it, R-precision with ``damsm_image_encoder``
    and an ``RNN_ENCODER``, the Kernel Inception Distance with ``kid`` (over ``kid_subsets`` subsets of ``kid_subset_size`` rows) and the
    Inception Score with ``inception_score`` = SPLITS > 0, both from the same Inception features; each is the keyword, else ``eval_opts``,
    else $XMC_FID_INCEPTION / $XMC_DAMSM_IMAGE_ENCODER; CLIPScore with ``clip_dir`` (a CLIP model directory; ``clip_max_tokens``: `CLIPScorer`'s
    ``max_tokens``, 64 unless ViT-B/16, L/14 or CLIP's own text context of 77 is wanted), from the caption strings of the
    batches (SENT captions, or WORD captions through the dataset's ``i2w``; 'clip_score_*' in ``metrics``).  With ``org_dir`` the real side is cached beside it.  Every score is logged (or one
    line says why there is none), written to ``writer`` and, FID apart, put into ``metrics`` when a dict is passed ('k' of PRDC as 'prdc_k';
    of KID and IS every name but 'kid' / 'inception_score' carries that word as a prefix: 'kid_std', 'kid_n_real', 'inception_score_n', ...).  Returns (uint8 tensor of the generated images,
    FID or None)."""
    from PIL import Image
    netG.eval()
    device = next(netG.parameters()).device
    if save_dir:
        os.makedirs(save_dir, exist_ok=True)
    save_org = False
    if org_dir:
        os.makedirs(org_dir, exist_ok=True)
        save_org = len(os.listdir(org_dir)) != num_samples
    given = eval_opts or EvalOptions()
    suite = MetricSuite(device, fid_inception or given.fid_inception or os.environ.get('XMC_FID_INCEPTION', ''),
                        given.prdc_k if prdc is None else prdc,
                        damsm_image_encoder or given.damsm_image_encoder or os.environ.get('XMC_DAMSM_IMAGE_ENCODER', ''), text_encoder,
                        **_new_metric_args(given, kid, kid_subsets, kid_subset_size, inception_score), **({'clip_dir': clip_dir, **_clip_tokens_arg(clip_max_tokens)} if clip_dir else {}))
    if org_dir:
        suite.open_cache(os.path.dirname(os.path.abspath(org_dir)))
    cnt, outs = 0, []
    for imgs, texts_lst, keys in loader:
        caps, cap_lens = texts_lst[0]
        words_embs, sent_embs, mask = encode(text_encoder, caps, cap_lens, keys)
        noise = torch.randn(sent_embs.size(0), cfg.TRAIN.NOISE_DIM).to(device)
        fake = netG(noise=noise, sent_embs=sent_embs, words_embs=words_embs, mask=mask)
        outs.append(((fake + 1.0) * 127.5).clamp(0, 255).to(torch.uint8).cpu())
        if clip_dir:
            suite.update_fake(fake, sent_embs, captions=_caption_strings(caps, cap_lens, loader))
        else:
            suite.update_fake(fake, sent_embs)
        suite.update_real(imgs)              # (taken only while a metric lacks its real side)
        for j in range(fake.size(0)):
            if save_dir:
                Image.fromarray(to_uint8_hwc(fake[j])).save(f'{save_dir}/{keys[j]}.png')
            if save_org:
                Image.fromarray(to_uint8_hwc(imgs[j])).save(f'{org_dir}/{keys[j]}.png')
        cnt += fake.size(0)
        if cnt >= num_samples:
            break
    suite.real_from_cache(cnt, lambda: (imgs for imgs, _, _ in loader))
    results = list(suite.results())
    if not results or results[0][0] != 'FID':     # no Inception weights: between the two directories, where pytorch_fid imports
        fid = fid_between(org_dir, save_dir, device) if (save_dir and org_dir and cnt) else None
        results.insert(0, ('FID', None if fid is None else dict(FID=fid), 'pytorch_fid is not installed'))
    fid = None
    for metric, values, why in results:
        line, tags, line_without = _EVAL_REPORT[metric]
        if values is None:
            logger.info(line_without.format(epoch=state_epoch, cnt=cnt, why=why))
            continue
        logger.info(line.format(epoch=state_epoch, **values))
        for key in tags:
            if writer is not None:
                writer.add_scalar(_EVAL_SCALAR.get(key, key), values[key], state_epoch)
        if metric == 'FID':
            fid = values['FID']
        elif metrics is not None:
            metrics.update({_EVAL_METRICS_KEY.get((metric, k), k): v for k, v in values.items()})
    return (torch.cat(outs) if outs else None), fid


def build_models(device):
    """netG / netD from the registries + the two Adam optimizers (train_gan.py:470-484)."""
    netG = _GEN_ARCH[cfg.GEN.ENCODER_NAME](cfg).to(device)
    netD = _DISC_ARCH[cfg.DISC.ENCODER_NAME](cfg, is_disc=True).to(device)
    if cfg.TRAIN.HE_INIT:
        netG.apply(weight_init)
        netD.apply(weight_init)
    O = cfg.TRAIN.OPT
    optimizerG = HipAdam(netG.parameters(), lr=O.G_LR, betas=(O.G_BETA1, O.G_BETA2))
    optimizerD = HipAdam(netD.parameters(), lr=O.D_LR, betas=(O.D_BETA1, O.D_BETA2))
    return netG, netD, optimizerG, optimizerD


def build_loaders(args, data_dir, device, seed, rank, world, logger):
    """(train_loader, test_loader or None): ``--synthetic`` batches, the device-resident ``--image_cache``, or the reference's loaders"""
    if args.synthetic > 0:
        return SyntheticCOCO(args.synthetic, cfg.TRAIN.BATCH_SIZE, cfg.IMG.SIZE, cfg.TEXT.MAX_LENGTH, seed, cfg.TEXT.VOCA_SIZE), None
    data_arch = _TEXT_DATASET[cfg.TEXT.TYPE]
    if args.image_cache:        # the same items out of a device-resident uint8 cache (xmc_gan_amd/imagecache.py): no image is opened here
        from xmc_gan_amd.imagecache import DeviceImageLoader, ImageCache
        loaders = {}
        for mode in ('train', 'test'):
            text_set = data_arch(data_dir=data_dir, mode=mode, transform=None, cfg=cfg)
            try:
                cache = ImageCache.load(args.image_cache, mode, cfg.IMG.SIZE, text_set.filenames, data_dir=data_dir)
            except ValueError as e:
                raise SystemExit(f'--image_cache: {e}')       # (the message ends with the command that builds this split's cache)
            loaders[mode] = DeviceImageLoader(cache, text_set, cfg.TRAIN.BATCH_SIZE, device, train=mode == 'train', seed=args.seed,
                                              rank=rank, world=world, start_epoch=args.resume_epoch)
            logger.info(f'image cache {cache.u8_path}: {len(cache)} images, {cache.nbytes} bytes on the device')
        return loaders['train'], loaders['test']
    # the reference's loaders (train_gan.py:440-457); each rank draws its own shuffled batches
    train_set = data_arch(data_dir=data_dir, mode='train', transform=train_transform(cfg.IMG.SIZE), cfg=cfg)
    test_set = data_arch(data_dir=data_dir, mode='test', transform=test_transform(cfg.IMG.SIZE), cfg=cfg)
    sampler = torch.utils.data.distributed.DistributedSampler(train_set, world, rank, shuffle=True, drop_last=True) \
        if world > 1 else None
    train_loader = torch.utils.data.DataLoader(train_set, batch_size=cfg.TRAIN.BATCH_SIZE, drop_last=True,
                                               shuffle=sampler is None, sampler=sampler,
                                               num_workers=int(cfg.TRAIN.NUM_WORKERS), pin_memory=True)
    test_loader = torch.utils.data.DataLoader(test_set, batch_size=cfg.TRAIN.BATCH_SIZE, drop_last=True, shuffle=False,
                                              num_workers=int(cfg.TRAIN.NUM_WORKERS))
    return train_loader, test_loader


def cached_text_encoder(args, data_dir, train_loader, test_loader, device, logger):
    """``--caption_cache``: the encoder's outputs out of device-resident tables (xmc_gan_amd/captioncache.py), no encoder is constructed;
    the train split's stand-in carries the test split's as ``eval_encoder``"""
    from xmc_gan_amd.captioncache import CachedTextEncoder, CaptionCache
    cached = {}
    for mode, loader in (('train', train_loader), ('test', test_loader)):
        text_set = loader.dataset
        if text_set.transform is not None:      # (the PIL loader's dataset: the same captions, read without its images)
            text_set = _TEXT_DATASET[cfg.TEXT.TYPE](data_dir=data_dir, mode=mode, transform=None, cfg=cfg)
        try:
            c_cache = CaptionCache.load(args.caption_cache, mode, cfg, text_set, ops.precision(), cfg_path=args.cfg)
        except ValueError as e:
            raise SystemExit(f'--caption_cache: {e}')     # (the message ends with the command that builds this split's cache)
        cached[mode] = CachedTextEncoder(c_cache, device)
        logger.info(f'caption cache {c_cache.f32_path}: {len(c_cache)} captions, {c_cache.nbytes} bytes on the device, {c_cache.encoder} encoder '
                    f'{c_cache.meta["encoder_fingerprint"]} from {c_cache.meta["encoder_source"]}')
    cached['train'].eval_encoder = cached['test']
    return cached['train']


def build_text_encoder(device, seed, synthetic=False, sbert_dir='', weights=None):
    """-> (the frozen text encoder in eval mode, whether it has its weights).  ``weights``: a state dict's path instead of TEXT.ENCODER_DIR;
    a ``synthetic`` run goes without the latter when the file is not there (random weights: the caller's to broadcast or to warn about)."""
    if synthetic and cfg.TEXT.ENCODER_NAME != 'RNN':
        return SyntheticTextEncoder(cfg.TEXT.EMBEDDING_DIM, cfg.TEXT.MAX_LENGTH, seed, device), True
    if cfg.TEXT.ENCODER_NAME == 'SBERT':
        # frozen weights read from the model directory, the same on every rank: no state dict to load (TEXT.ENCODER_DIR is '' in every
        # SBERT preset and the reference never loads one), no parameters to broadcast or freeze
        return SBERT_ENCODER(cfg=cfg, model_dir=sbert_dir or None).to(device).eval(), True
    text_encoder = _TEXT_ARCH[cfg.TEXT.ENCODER_NAME](cfg=cfg).to(device)        # train_gan.py:459-468
    path = weights if weights is not None else (f'{PROJ_DIR}/{cfg.TEXT.ENCODER_DIR}' if cfg.TEXT.ENCODER_DIR else '')
    loaded = bool(path) and (weights is not None or not synthetic or os.path.isfile(path))
    if loaded:
        text_encoder.load_state_dict(torch.load(path, map_location=device))
    for p_ in text_encoder.parameters():
        p_.requires_grad = False
    return text_encoder.eval(), loaded


def _checked_args(argv):
    """-> (args, the --diffaug policy, EvalOptions): everything that can be refused before a device is touched; reads the cfg and applies
    the flags that override it"""
    args = parse_args(argv)
    if not 0.0 <= args.ema_decay < 1.0 or args.ema_start < 0:
        raise SystemExit('--ema_decay must be in [0, 1) and --ema_start >= 0')
    try:
        aug_policy = parse_policy(args.diffaug)
    except ValueError as e:
        raise SystemExit(f'--diffaug: {e}')
    if args.image_cache and args.synthetic > 0:
        raise SystemExit('--image_cache and --synthetic exclude each other')
    if args.caption_cache and args.synthetic > 0:
        raise SystemExit('--caption_cache and --synthetic exclude each other')
    cfg_from_file(args.cfg)
    if args.imsize != -1:
        cfg.IMG.SIZE = args.imsize
    if args.bs != -1:
        cfg.TRAIN.BATCH_SIZE = args.bs
    if args.max_epoch != -1:
        cfg.TRAIN.MAX_EPOCH = args.max_epoch
    if args.precision:
        ops.set_precision(args.precision)
    # the VGG term's weights: refused here, at start-up, and not at the first generator step.  Without the switch nothing is looked for
    args.vgg_weights = resolve_vgg_weights(args.vgg_weights) if cfg.TRAIN.ENCODER_LOSS.VGG else ''
    if cfg.TRAIN.ENCODER_LOSS.VGG and cfg.IMG.SIZE % 32:
        raise SystemExit(f'TRAIN.ENCODER_LOSS.VGG: five 2x2 pools need an image size that is a multiple of 32, got {cfg.IMG.SIZE}')
    fid_inception = resolve_weights(args.fid_inception, 'XMC_FID_INCEPTION', '--fid_inception', must_exist=False)
    if not 0 <= args.prdc <= 16:
        raise SystemExit('--prdc K: 0 (off) or 1 <= K <= 16 nearest neighbours')
    if args.kid_subsets < 1 or args.kid_subset_size < 2:
        raise SystemExit('--kid_subsets S >= 1 and --kid_subset_size M >= 2')
    if args.inception_score < 0:
        raise SystemExit('--inception_score SPLITS: 0 (off) or a positive number of parts')
    eval_opts = EvalOptions(fid_inception, args.prdc,
                            resolve_weights(args.damsm_image_encoder, 'XMC_DAMSM_IMAGE_ENCODER', '--damsm_image_encoder', must_exist=False),
                            args.kid, args.kid_subsets, args.kid_subset_size, args.inception_score)
    args.clip_dir = args.clip_dir or os.environ.get('XMC_CLIP_DIR', '')
    if not 64 <= args.clip_max_tokens <= 1024:
        raise SystemExit(f'--clip_max_tokens: {args.clip_max_tokens} is outside [64, 1024]')
    if args.clip_dir and not os.path.isfile(os.path.join(args.clip_dir, 'config.json')):
        raise SystemExit(f'--clip_dir: {args.clip_dir} is not a CLIP model directory (no config.json)')
    return args, aug_policy, eval_opts


def _init_process(args):
    """-> (device, rank, world): this process's card and, under ``torch.distributed.run``, the process group"""
    world = int(os.environ.get('WORLD_SIZE', '1'))
    local_rank = int(os.environ.get('LOCAL_RANK', str(args.gpu_id)))
    if not torch.cuda.is_available():
        raise RuntimeError('xmc_gan/train_gan.py needs an MI355X (HIP kernels only; the CPU restatement lives in oracle/)')
    # one process per GPU over RCCL ('nccl'); XMC_DIST_BACKEND=gloo is the one-card rehearsal of the same code (ranks share card 0 when
    # there are fewer cards than ranks; tests/test_parallel_gpu.py)
    backend = os.environ.get('XMC_DIST_BACKEND', 'nccl')
    if backend != 'nccl':
        local_rank %= max(1, torch.cuda.device_count())
    torch.cuda.set_device(local_rank)
    device = torch.device('cuda', local_rank)
    if world > 1:
        torch.distributed.init_process_group(backend)
    return device, parallel.rank(), world


def main(argv=None):
    args, aug_policy, eval_opts = _checked_args(argv)
    device, rank, world = _init_process(args)
    seed = args.seed + rank
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)

    output_dir = args.output_dir or f'{PROJ_DIR}/output/{cfg.DATASET_NAME}{cfg.IMG.SIZE}_{cfg.CONFIG_NAME}_{args.seed}'
    img_dir, log_dir, model_dir = output_dir + '/img', output_dir + '/log', output_dir + '/model'
    if rank == 0:
        for d_ in (output_dir, img_dir, log_dir, model_dir):
            os.makedirs(d_, exist_ok=True)
    logger = setup_logger(name=cfg.CONFIG_NAME, save_dir=log_dir if rank == 0 else None, distributed_rank=rank)
    logger.info('Using config:')
    logger.info(cfg)
    logger.info(f'seed now is : {args.seed}')

    data_dir = args.data_dir or f'{PROJ_DIR}/data/{cfg.DATASET_NAME}'
    train_loader, test_loader = build_loaders(args, data_dir, device, seed, rank, world, logger)
    if args.caption_cache:
        text_encoder = cached_text_encoder(args, data_dir, train_loader, test_loader, device, logger)
    else:
        text_encoder, has_weights = build_text_encoder(device, seed, args.synthetic > 0, args.sbert_dir)
        if not has_weights and world > 1:       # random (synthetic-run) encoder weights must agree across ranks
            for p_ in text_encoder.parameters():
                torch.distributed.broadcast(p_.data, 0)

    netG, netD, optimizerG, optimizerD = build_models(device)
    if world > 1:   # same initial weights (and spectral-norm u/v vectors, which then evolve identically) on every rank
        for p_ in list(netG.parameters()) + list(netD.parameters()) + list(netG.buffers()) + list(netD.buffers()):
            torch.distributed.broadcast(p_.data, 0)
    logger.info(f'netG # of parameters: {count_params(netG)}')
    logger.info(f'netD # of parameters: {count_params(netD)}')

    state_epoch = args.resume_epoch
    if state_epoch != 0:
        load_checkpoint(model_dir, state_epoch, netG, netD, optimizerG, optimizerD, device=device, logger=logger)
    elif cfg.DISC.ENCODER_DIR:
        netD.load_state_dict(torch.load(f'{PROJ_DIR}/{cfg.DISC.ENCODER_DIR}', map_location=device), strict=False)

    # the generator's weight average (--ema_decay > 0): after the broadcast / the resume, so that it starts from the weights in use
    ema = None
    if args.ema_decay > 0:
        ema = ParamEMA(netG, args.ema_decay, args.ema_start)
        logger.info(f'generator weight EMA: decay {ema.decay}, averaging after {ema.start} generator steps')
        if state_epoch != 0:
            load_average(model_dir, state_epoch, ema, device, logger)

    # augmentation of the discriminator's inputs (--diffaug): one sampler, created before any capture.  Its draws come from (seed, rank) and,
    # on a resume, from (seed, rank, epoch): a resumed run does not continue the interrupted run's draws, it starts a stream of its own
    aug = None
    if aug_policy:
        aug = DiffAugment(','.join(aug_policy), cfg.TRAIN.BATCH_SIZE, cfg.IMG.SIZE, cfg.IMG.SIZE, device, args.seed, rank)
        if state_epoch != 0:
            aug.seed(args.seed, rank, state_epoch)
        logger.info(f'DiffAugment on the discriminator inputs: {",".join(aug.policy)}')

    # the frozen VGG-19 of TRAIN.ENCODER_LOSS.VGG: held by the step options, not by netG / netD (nothing of it reaches a checkpoint); its
    # packed weights are made here, before any capture
    vgg = None
    if cfg.TRAIN.ENCODER_LOSS.VGG:
        vgg = VGGContrast(VGG19Features(args.vgg_weights, device).warm())
        logger.info(f'VGG-19 image-image contrastive term: weights {args.vgg_weights}, weight {args.vgg_smooth}')

    writer = ScalarLog(log_dir, args.log_type, run_name=cfg.CONFIG_NAME) if rank == 0 else None
    last = train(train_loader=train_loader, test_loader=test_loader, state_epoch=state_epoch, text_encoder=text_encoder,
                 netG=netG, netD=netD, optimizerG=optimizerG, optimizerD=optimizerD, logger=logger, model_dir=model_dir,
                 opts=StepOptions(gather_negatives=args.gather_negatives, graph=bool(args.graph), log_each_step=bool(args.log_each_step),
                                  ema=ema, diffaug=aug, vgg=vgg, vgg_smooth=args.vgg_smooth),
                 img_dir=img_dir if rank == 0 else None, writer=writer, eval_opts=eval_opts, clip_dir=args.clip_dir or None,
                 **_clip_tokens_arg(args.clip_max_tokens))
    if writer is not None:
        writer.close()
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.destroy_process_group()
    main.last_ema = ema                      # (None without --ema_decay)
    main.last_models = (netG, netD)          # (for callers that drive main() in-process: the tests compare runs by their final weights)
    return last


if __name__ == '__main__':
    main()
