"""R-precision on the device: does a generated image retrieve its own caption?  AttnGAN's protocol, the second number the DF-GAN /
AttnGAN family reports beside FID; the reference has no such evaluation.

For every image, the cosine between its DAMSM image code (``xmc_gan.model.encoder.CNN_ENCODER``, the ``cnn_code``) and the sentence codes
(``RNN_ENCODER``'s ``sent_embs``) of ``k`` candidate captions -- its own and ``k - 1`` drawn from the captions of other images -- is
ranked; the image is a hit when its own caption comes first.  R-precision is the mean hit rate, in percent, over ``splits`` contiguous parts
of the image list, and its spread is the standard deviation over those parts.

The candidates are drawn on the host (`candidate_table`, a seeded numpy Generator); cosines and ranks come from one launch of
``xmc_rprecision`` (csrc/retrieval.hip) on the code rows, which stay on the device.  The weights of the image encoder are a file the user
supplies (``image_encoder100.pth`` of AttnGAN's DAMSM archive; ``XMC_DAMSM_IMAGE_ENCODER``).

Agreement with AttnGAN's own evaluation on the real weights file has not been checked (neither the file nor torchvision is available where
this was written); what is checked is agreement with the plain-torch f64 restatement in tests/damsm_ref.py.
"""
import os

import numpy as np
import torch

from . import ops

ENV = "XMC_DAMSM_IMAGE_ENCODER"


def load_image_encoder(path=None, nef=None, device="cuda"):
    """``CNN_ENCODER(nef)`` with the state dict of ``path`` (default: $XMC_DAMSM_IMAGE_ENCODER) on ``device``, in evaluation mode.  ``nef``
    None: taken from the file.  A ``module.`` prefix on every key is accepted, ``num_batches_tracked`` entries may be missing (checkpoints
    written before PyTorch 0.4.1 have none), other keys are ignored.  ImportError: no path, no file, a missing key; ValueError: a wrong shape."""
    from xmc_gan.model.encoder import CNN_ENCODER
    from .fid import check_inception_state
    path = path or os.environ.get(ENV, "")
    if not path:
        raise ImportError("R-precision needs the DAMSM image encoder (image_encoder100.pth of AttnGAN's DAMSM archive, the file beside "
                          f"text_encoder100.pth): pass its path / --damsm_image_encoder / --image_encoder or set {ENV}.  None is given.")
    if not os.path.isfile(path):
        raise ImportError(f"CNN_ENCODER: the weights file {path} does not exist")
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ImportError(f"CNN_ENCODER: {path} holds a {type(sd).__name__}, a state dict was expected")
    if len(sd) and all(k.startswith("module.") for k in sd):
        sd = {k[len("module."):]: v for k, v in sd.items()}
    check_inception_state(sd, "CNN_ENCODER", path)
    for key in ("emb_features.weight", "emb_cnn_code.weight", "emb_cnn_code.bias"):
        if key not in sd:
            raise ImportError(f"CNN_ENCODER: the weights in {path} lack {key!r}")
    w = sd["emb_cnn_code.weight"]
    if w.dim() != 2 or w.shape[1] != 2048:
        raise ValueError(f"CNN_ENCODER: emb_cnn_code.weight is {tuple(w.shape)}, [nef, 2048] expected")
    nef = int(w.shape[0]) if nef is None else int(nef)
    for key, shape in (("emb_features.weight", (nef, 768, 1, 1)), ("emb_cnn_code.weight", (nef, 2048)), ("emb_cnn_code.bias", (nef,))):
        if tuple(sd[key].shape) != shape:
            raise ValueError(f"CNN_ENCODER: {key} is {tuple(sd[key].shape)}, nef = {nef} needs {shape}")
    enc = CNN_ENCODER(nef)
    own = enc.state_dict()
    enc.load_state_dict({k: sd.get(k, v) for k, v in own.items()}, strict=True)
    return enc.to(device).eval()


def candidate_table(caption_of_image, group_of_caption, k=100, seed=0):
    """int32 [N, k]: column 0 is ``caption_of_image[n]``; columns 1..k-1 are distinct captions drawn uniformly from the captions whose group
    differs from that caption's (``group_of_caption[m]``: the image a caption was written for; the captions of one image form a group).
    Host work with ``np.random.default_rng(seed)``: the same seed gives the same table.  ValueError: fewer than k - 1 captions of other
    groups exist for some image."""
    own = np.asarray(caption_of_image, dtype=np.int64).reshape(-1)
    group = np.asarray(group_of_caption, dtype=np.int64).reshape(-1)
    N, M, k = own.size, group.size, int(k)
    if k < 1 or N < 1 or M < 1:
        raise ValueError(f"candidate_table: k = {k}, {N} images, {M} captions")
    if own.min() < 0 or own.max() >= M:
        raise ValueError(f"candidate_table: caption_of_image spans [{own.min()}, {own.max()}], there are {M} captions")
    # captions sorted by group: the captions of other groups are everything but one contiguous run [lo, hi) of that order
    order = np.argsort(group, kind="stable")
    sorted_groups = group[order]
    lo = np.searchsorted(sorted_groups, group[own], side="left")
    hi = np.searchsorted(sorted_groups, group[own], side="right")
    others = M - (hi - lo)
    if k > 1 and others.min() < k - 1:
        raise ValueError(f"candidate_table: k = {k} needs {k - 1} captions of other groups, an image has only {int(others.min())}")
    rng = np.random.default_rng(seed)
    table = np.empty((N, k), dtype=np.int32)
    table[:, 0] = own
    for n in range(N if k > 1 else 0):
        pick = rng.choice(int(others[n]), size=k - 1, replace=False)
        table[n, 1:] = order[np.where(pick < lo[n], pick, pick + (hi[n] - lo[n]))]
    return table


def split_statistics(hits, splits=10):
    """(mean, std, per-split rates) in percent of a 0/1 hit vector over ``splits`` contiguous parts of n // splits images; the last
    n % splits images are counted in the last part (AttnGAN's protocol: mean and np.std of the per-split rates)"""
    hits = np.asarray(hits, dtype=np.float64).reshape(-1)
    n, splits = hits.size, int(splits)
    if splits < 1 or n < splits:
        raise ValueError(f"R-precision over {splits} splits needs at least {max(splits, 1)} images, got {n}")
    step = n // splits
    rates = np.array([100.0 * hits[i * step:((i + 1) * step if i + 1 < splits else n)].mean() for i in range(splits)])
    return float(rates.mean()), float(rates.std()), rates


class RPrecision:
    """Accumulates image and caption code rows on the device; `finalize` draws the candidate table, ranks with one kernel launch and returns
    dict(r_precision, std, n, k, splits, per_split)."""

    def __init__(self, k=100, splits=10, seed=0):
        if k < 2 or splits < 1:
            raise ValueError(f"RPrecision: k = {k} (>= 2), splits = {splits} (>= 1)")
        self.k, self.splits, self.seed = int(k), int(splits), int(seed)
        self._img, self._txt, self._own = [], [], []
        self.n = self.m = 0

    def update(self, image_codes, caption_codes, caption_of_image=None):
        """image_codes f32 [B,D], caption_codes f32 [C,D] on the device.  ``caption_of_image`` None: B == C and image i was made from
        caption i; else int [B], rows of THIS call's ``caption_codes`` (several images of one caption)."""
        img, txt = image_codes.detach().float(), caption_codes.detach().float()
        if img.dim() != 2 or txt.dim() != 2 or img.shape[1] != txt.shape[1]:
            raise ValueError(f"RPrecision.update: code rows [B,D] and [C,D] expected, got {tuple(img.shape)} and {tuple(txt.shape)}")
        if caption_of_image is None:
            if img.shape[0] != txt.shape[0]:
                raise ValueError(f"RPrecision.update: {img.shape[0]} images and {txt.shape[0]} captions need a caption_of_image")
            own = np.arange(img.shape[0], dtype=np.int64)
        else:
            own = np.asarray(torch.as_tensor(caption_of_image).cpu(), dtype=np.int64).reshape(-1)
            if own.size != img.shape[0] or (own.size and (own.min() < 0 or own.max() >= txt.shape[0])):
                raise ValueError("RPrecision.update: caption_of_image must name a row of caption_codes for every image")
        self._img.append(img.clone()), self._txt.append(txt.clone()), self._own.append(own + self.m)
        self.n += img.shape[0]
        self.m += txt.shape[0]

    def hits(self):
        """(0/1 hit per image as a numpy array, the candidate table)"""
        if self.n < 1:
            raise ValueError("RPrecision: no image was given")
        own = np.concatenate(self._own)
        table = candidate_table(own, np.arange(self.m), self.k, self.seed)         # every caption row a group of its own
        img, txt = torch.cat(self._img).contiguous(), torch.cat(self._txt).contiguous()
        rank = ops.rprecision(img, txt, torch.from_numpy(table))
        return (rank.cpu().numpy() == 0).astype(np.int64), table

    def finalize(self):
        hits, _ = self.hits()
        mean, std, rates = split_statistics(hits, self.splits)
        return dict(r_precision=mean, std=std, n=int(hits.size), k=self.k, splits=self.splits, per_split=[float(r) for r in rates])


def usable_with(text_encoder, image_encoder):
    """None when ``text_encoder``'s sentence codes live in ``image_encoder``'s space (an RNN_ENCODER of the same width, or a
    `CachedTextEncoder` whose cache was built by one), else the reason"""
    from xmc_gan.model.encoder import RNN_ENCODER
    from .captioncache import CachedTextEncoder
    if isinstance(text_encoder, CachedTextEncoder):
        if text_encoder.encoder_name != "RNN":
            return f"the caption cache was built by a {text_encoder.encoder_name} encoder, the DAMSM image encoder is paired with RNN_ENCODER"
        width = text_encoder.emb_dim
    elif not isinstance(text_encoder, RNN_ENCODER):
        return f"the text encoder is a {type(text_encoder).__name__}, the DAMSM image encoder is paired with RNN_ENCODER"
    else:
        width = text_encoder.nhidden * text_encoder.num_directions
    if width != image_encoder.nef:
        return f"TEXT.EMBEDDING_DIM is {width}, the image encoder's nef is {image_encoder.nef}"
    return None
