"""The evaluation pipeline behind ``train_gan.eval()``, ``sample.py`` and the scoring command lines ("The evaluation pipeline"):
where a metric's weights come from, the loaded models, and ``MetricSuite`` -- FID, precision / recall / density / coverage (PRDC),
R-precision, KID, the Inception Score and CLIPScore over one pass of the images.  Nothing but ``os`` is imported until a metric is asked for."""
import os

FID, PRDC, RPREC, KID, IS = "FID", "PRDC", "R-precision", "KID", "IS"
CLIP = "CLIPScore"
CACHE_FILES = {FID: "org_stats.npz", PRDC: "org_features.npz", KID: "org_features.npz"}       # eval()'s real side, beside org_dir (PRDC and KID: one file)
_WHAT = {"XMC_FID_INCEPTION": "FID Inception weights", "XMC_DAMSM_IMAGE_ENCODER": "DAMSM image encoder weights"}
_models = {}            # 'inception' / 'damsm' / 'clip' -> (key, model): one loaded model per kind (`load_model`)


def resolve_weights(given, env_name, flag, must_exist=True, refusal=None):
    """(Refusable before a device is touched.)  The weights file of a metric: ``given`` (the value of ``flag``), else $``env_name``.  Without
    either: '' when ``must_exist`` is false (the metric is off), else SystemExit; no file: SystemExit.  ``refusal``: the opening of the one
    message for both, which shows what was got."""
    path = given or os.environ.get(env_name, "")
    if refusal is not None:
        if not path or not os.path.isfile(path):
            raise SystemExit(f"{refusal}: {flag} PATH or {env_name} (got {path!r})")
    elif not path:
        if must_exist:
            raise SystemExit(f"scoring a directory needs the {_WHAT[env_name]}: {flag} PATH or {env_name}")
    elif not os.path.isfile(path):
        raise SystemExit(f"{flag}: {path} is not a file")
    return path


def image_set_kind(path):
    """'dir' (an image directory), 'npz' (a statistics or feature file) or None"""
    return "dir" if os.path.isdir(path) else "npz" if os.path.isfile(path) and path.endswith(".npz") else None


def load_model(kind, path, device, max_tokens=64):
    """the Inception extractor ('inception') or DAMSM image encoder ('damsm') of a weights file, or the CLIP scorer ('clip') of a model
    directory: one per kind, reloaded when the file (the directory's config.json), its modification time, the device or ``max_tokens``
    (`CLIPScorer`'s longest sequence; read for 'clip' only) is another"""
    import torch
    stamp = os.path.join(path, "config.json") if kind == "clip" else path
    key = (os.path.abspath(path), os.stat(stamp).st_mtime_ns if os.path.isfile(stamp) else None, str(torch.device(device)))
    if kind == "clip":
        key += (int(max_tokens),)
    if _models.get(kind, (None, None))[0] != key:
        _models.pop(kind, None)
        if kind == "inception":
            from . import fid as F
            _models[kind] = key, F.InceptionFID(path, device)
        elif kind == "clip":
            from . import clip as CL
            _models[kind] = key, CL.CLIPScorer(path, device, int(max_tokens))
        else:
            from . import rprecision as RP
            _models[kind] = key, RP.load_image_encoder(path, None, device)
    return _models[kind][1]


class MetricSuite:
    """FID (``fid``) and PRDC (``prdc_k`` > 0) with the Inception weights ``fid_inception``, R-precision with the DAMSM weights
    ``damsm_image_encoder`` and a ``text_encoder`` it is paired with; ``why``: the reason of every metric that was asked for and cannot run.
    The generated side comes through ``update_fake``; the real side of FID and PRDC from ``update_real`` while ``wants_real``, from
    ``real_from_path``, or from the cache files that ``open_cache`` reads and ``real_from_cache`` settles.  The cache rule: a file is reused
    if and only if it was made from as many images as were generated now; otherwise the real side is the rows ``update_real`` gathered -- or,
    where a file for another count kept them from being gathered, those of one more pass over the real images -- and is written.
    ``kid``: the Kernel Inception Distance over ``kid_subsets`` subsets of ``kid_subset_size`` rows; it is two-sided, takes the feature rows
    and shares PRDC's bank and cache file: with both on, the rows are stored, read and written once.  ``inception_score`` > 0: the Inception
    Score over that many splits, one-sided like R-precision.  ``clip_dir``: CLIPScore with the CLIP model directory there, one-sided, from the
    caption strings ``update_fake`` is given; ``clip_max_tokens`` is `CLIPScorer`'s ``max_tokens`` (64: ViT-B/32 at a text context of 64)."""

    def __init__(self, device, fid_inception="", prdc_k=0, damsm_image_encoder="", text_encoder=None, rp_k=100, rp_splits=10, rp_seed=0, fid=True,
                 kid=False, kid_subsets=100, kid_subset_size=1000, kid_seed=0, inception_score=0, clip_dir="", clip_max_tokens=64):
        self.device, self.prdc_k, self.why = device, int(prdc_k), {}
        self.kid_args, is_splits = (int(kid_subsets), int(kid_subset_size), int(kid_seed)), int(inception_score)
        self.extractor = self.encoder = self._cache_dir = None
        self.fake = {}                                              # metric -> its accumulator of the generated side: the metrics that are on
        self._gathered, self._cached, self.real = {}, {}, {}        # FID / PRDC -> real accumulator; (what a cache file held, n); () -> real side
        if fid_inception and (fid or self.prdc_k > 0 or kid or is_splits > 0):
            self.extractor = load_model("inception", fid_inception, device)
            if fid:
                from .fid import FeatureStats
                self.fake[FID] = FeatureStats(device=device)
            if self.prdc_k > 0:
                from .manifold import FeatureBank
                self.fake[PRDC] = FeatureBank(device=device)
            if kid:
                from .manifold import FeatureBank
                self.fake[KID] = self.fake[PRDC] if PRDC in self.fake else FeatureBank(device=device)       # one bank of rows for both
            if is_splits > 0:
                from .fid import InceptionScore
                try:
                    self.fake[IS] = InceptionScore(self.extractor, is_splits, device)
                except ValueError as e:                     # (the weights file holds no classifier)
                    self.why[IS] = str(e)
        else:
            for m, on in ((PRDC, self.prdc_k > 0), (KID, kid), (IS, is_splits > 0)):
                if on:
                    self.why[m] = "it takes the Inception features of FID: --fid_inception PATH or XMC_FID_INCEPTION"
        if damsm_image_encoder:
            from . import rprecision as RP
            self.encoder = load_model("damsm", damsm_image_encoder, device)
            why = RP.usable_with(text_encoder, self.encoder)
            if why is None:
                self.fake[RPREC] = RP.RPrecision(rp_k, rp_splits, rp_seed)
            else:
                self.why[RPREC] = why
        if clip_dir:
            from .clip import CLIPScoreStats
            more = {} if int(clip_max_tokens) == 64 else {"max_tokens": int(clip_max_tokens)}      # off: the call it was
            self.fake[CLIP] = CLIPScoreStats(load_model("clip", clip_dir, device, **more))
        self._rows = PRDC if PRDC in self.fake else KID                # the metric the bank of rows and its real side are kept under
        self._two_sided = [m for m in (FID, self._rows) if m in self.fake]

    def _u8(self, images):
        """[B,3,H,W] floats in [-1, 1] -> the uint8 [B,H,W,3] the PNGs hold; uint8 images are taken as they are"""
        import torch
        from . import fid as F
        return images if images.dtype == torch.uint8 else F.nchw_to_u8(images.to(self.device))

    def _feed_real(self, images, metrics):
        feats = self.extractor(self._u8(images))
        for m in metrics:
            if m not in self._gathered:
                self._gathered[m] = type(self.fake[m])(device=self.device)
            self._gathered[m].update(feats)

    def update_fake(self, images, sent_embs=None, caption_of_image=None, captions=None):
        """generated images ([B,3,H,W] floats or uint8 [B,H,W,3]); for R-precision their sentence codes and, where images share one, each image's
        row; for CLIPScore their caption strings (one per image, or fewer and each image's row): a batch without them is not scored"""
        if not self.fake:
            return
        u8 = self._u8(images)
        if self._two_sided or IS in self.fake:
            feats = self.extractor(u8)
            for m in self._two_sided + [IS] * (IS in self.fake):
                self.fake[m].update(feats)
        if RPREC in self.fake:
            self.fake[RPREC].update(self.encoder.encode_u8(u8)[1], sent_embs, caption_of_image)
        if CLIP in self.fake and captions is not None:
            self.fake[CLIP].update(u8, captions, caption_of_image)

    @property
    def wants_real(self):
        """the metrics that are on and still lack their real side (none: empty, false)"""
        return [m for m in self._two_sided if m not in self.real and m not in self._cached]

    def update_real(self, images):
        """a batch of real images, for the metrics that still lack their real side"""
        if self.wants_real:
            self._feed_real(images, self.wants_real)

    def real_from_path(self, fid_path=None, prdc_path=None, batch=100, kid_path=None):
        """FID's real side (an image directory or an .npz statistics file), PRDC's and KID's (a directory or a feature file each; the same
        path is read once), read by ``results()``"""
        if FID in self.fake:
            from .fid import stats_of
            self.real[FID] = lambda: stats_of(fid_path, self.extractor, batch)
        banks = {}

        def bank(path):
            from .manifold import bank_of
            if path not in banks:
                banks[path] = bank_of(path, self.extractor, batch, self.device)
            return banks[path]
        if PRDC in self.fake:
            self.real[PRDC] = lambda: bank(prdc_path)
        if KID in self.fake:
            self.real[KID] = lambda: bank(kid_path)

    def open_cache(self, cache_dir):
        """before the first batch: ``cache_dir`` holds (or will hold) the real side's files; a feature file that does not read counts as absent"""
        self._cache_dir = cache_dir
        for m in self._two_sided:
            path = os.path.join(cache_dir, CACHE_FILES[m])
            if os.path.isfile(path) and m == FID:
                from .fid import load_stats
                *stats, n = load_stats(path, with_count=True)
                self._cached[m] = stats, n
            elif os.path.isfile(path):
                from .manifold import FeatureBank
                try:
                    bank = FeatureBank.load(path, self.device)
                    self._cached[m] = bank, bank.n
                except ValueError:
                    pass

    def real_from_cache(self, count, refill):
        """after the last batch: the cache rule for ``count`` generated images; ``refill()`` (for a file of another count): the real batches again"""
        stale = [m for m in self._two_sided if m in self._cached and self._cached[m][1] != count]
        for images in (refill() if stale else ()):
            self._feed_real(images, stale)
            if min(self._gathered[m].n for m in stale) >= count:
                break
        for m in self._two_sided:
            if m in self._cached and m not in stale:
                self.real[m] = lambda value=self._cached[m][0]: value
            elif m not in self.real:
                acc = self._gathered[m] if m in self._gathered else type(self.fake[m])(device=self.device)
                if self._cache_dir and acc.n >= (2 if m == FID else 1):         # (a covariance needs two rows)
                    acc.save(os.path.join(self._cache_dir, CACHE_FILES[m]))
                self.real[m] = acc.finalize if m == FID else (lambda bank=acc: bank)

    def _prdc(self):
        from . import manifold as MF          # (`prdc` is looked up on the module when it is called)
        return MF.prdc(self.real[PRDC](), self.fake[PRDC], self.prdc_k)

    def _kid(self):
        from . import manifold as MF
        subsets, size, seed = self.kid_args
        return MF.kid(self.real[KID if KID in self.real else self._rows](), self.fake[KID], subsets, size, seed)

    def results(self):
        """yields (metric, values or None, why not or None) for every metric asked for, in the order FID, PRDC, R-precision, KID, IS, CLIPScore; values:
        dict(FID=x), `manifold.prdc`'s dict, `RPrecision.finalize`'s dict, `manifold.kid`'s dict, `InceptionScore.finalize`'s dict,
        `CLIPScoreStats.finalize`'s dict.  A
        ValueError of theirs is the reason."""
        if FID in self.fake and self.fake[FID].n < 2:
            yield FID, None, "fewer than two images"
        elif FID in self.fake:
            from .fid import frechet_distance
            yield FID, dict(FID=frechet_distance(*self.real[FID](), *self.fake[FID].finalize())), None
        for metric, compute in ((PRDC, self._prdc), (RPREC, lambda: self.fake[RPREC].finalize()), (KID, self._kid),
                                (IS, lambda: self.fake[IS].finalize()), (CLIP, lambda: self.fake[CLIP].finalize())):
            values, why = None, self.why.get(metric)
            if metric in self.fake:
                try:
                    values = compute()
                except ValueError as e:
                    why = str(e)
            if values is not None or why is not None:
                yield metric, values, why
