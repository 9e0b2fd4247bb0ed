"""The text encoder's outputs from a device-resident cache of caption embeddings (``train_gan.py --caption_cache DIR``).

The text encoders are frozen and in eval mode, ``TextDataset.__getitem__`` always hands out caption ``idx * CAPTIONS_PER_IMAGE + 1`` and
``get_caption`` is deterministic: a run encodes the same captions with the same weights in every epoch.  `build_cache` runs the encoder ONCE
over that one caption per image and stores what it returned; `CachedTextEncoder` uploads the two tables once and makes a batch's
``(words_embs, sent_embs, mask)`` with one launch (`ops.caption_gather`, csrc/captionfeed.hip).  A training run then needs neither the
encoder's weights nor, for SBERT, the RoBERTa directory and the ``tokenizers`` package.

Format (version 1), two files per split:

  ``<split>.cap.f32``      raw little-endian f32: the sentence rows [N, E] in the order of ``<data_dir>/<split>/filenames.pickle``, then the
                           token rows: for caption i, ``lens[i]`` rows of E floats starting at row ``tok_offsets[i]``.  Only the VALID tokens
                           are stored -- both encoders return exact zeros at t >= len, which the builder asserts on every batch -- and the
                           values are the encoder's f32 outputs, unrounded.  E % 4 == 0, so every row starts on a 16-byte boundary.
  ``<split>.cap.idx.npz``  ``lens`` int32 [N] (from the mask the encoder returned: SBERT's token count with <s> and </s>, the RNN's count of
                           non-zero ids), ``tok_offsets`` int64 [N], ``keys`` [N], ``version``, ``split``, ``emb_dim``, ``max_length``,
                           ``encoder`` ('SBERT' / 'RNN'), ``rnn_type``, ``bert_norm``, ``pooling``, ``precision`` (the engine's mode while
                           encoding), ``batch_size``, ``captions_fingerprint`` (sha256 over the captions handed out, in order),
                           ``encoder_fingerprint`` (sha256 over name, dtype, shape and bytes of the encoder's tensors in sorted name order),
                           ``encoder_source`` (where the weights came from)

Equal row counts.  The builder fills the last batch up to the batch size with captions it has already encoded and drops the filler's outputs:
every launch of the encoder then has the same number of rows.  The generic GEMM picks its tile by the row count and nothing promises the
same bits across tiles; a cache built at the run's batch size is compared bit for bit with the live encoder (tests/test_captioncache_gpu.py).

Out of scope: all CAPTIONS_PER_IMAGE captions of an image or a random choice among them, ``b_local``, 16-bit storage of the token rows,
tables in host memory or sharded over ranks (every rank holds both, as it holds the image pool), writing straight into the captured graph's
static inputs, caches for sample.py, encoders that are fine-tuned.
"""
import hashlib
import os

import numpy as np
import torch

FORMAT_VERSION = 1
UPLOAD_CHUNK = 256 << 20           # bytes per host-to-device copy of the tables
DEFAULT_RESERVE = 8 << 30          # device memory the upload leaves free for the training step
RANDOM_SOURCE = "<random initialisation>"
_META = ("emb_dim", "max_length", "encoder", "rnn_type", "bert_norm", "pooling")


def cache_paths(cache_dir, split):
    stem = os.path.join(cache_dir, f"{split}.cap")
    return stem + ".f32", stem + ".idx.npz"


def build_command(cfg_path, data_dir, split, cache_dir, precision=None):
    prec = f" --precision {precision}" if precision else ""
    return f"python xmc_gan/caption_cache.py build --cfg {cfg_path} --data_dir {data_dir} --split {split} --out {cache_dir}{prec}"


def cfg_meta(cfg):
    """what of ``cfg.TEXT`` decides the encoder's output: the fields a cache records and `CaptionCache.load` compares"""
    t = cfg.TEXT
    name = str(t.ENCODER_NAME)
    return dict(emb_dim=int(t.EMBEDDING_DIM), max_length=int(t.MAX_LENGTH), encoder=name,
                rnn_type=str(t.RNN_TYPE) if name == "RNN" else "", bert_norm=bool(t.BERT_NORM) if name == "SBERT" else False,
                pooling=str(t.POOLING_MODE) if name == "SBERT" else "")


def handed_out_captions(text_dataset):
    """[(caption, length)] in ``filenames`` order: the one caption per image ``TextDataset.__getitem__`` hands out (``sent_ix = 1``)"""
    per = text_dataset.caps_per_image
    return [text_dataset.get_caption(i * per + 1) for i in range(len(text_dataset.filenames))]


def captions_fingerprint(captions):
    """sha256 (hex) over `handed_out_captions`' list: a sentence as its UTF-8 bytes, token ids as their int64 bytes, each with its length"""
    h = hashlib.sha256()
    for cap, n in captions:
        if isinstance(cap, str):
            b = cap.encode("utf-8")
            h.update(b"S%d:%d:" % (int(n), len(b)) + b)
        else:
            a = np.ascontiguousarray(np.asarray(cap), dtype=np.int64)
            h.update(b"W%d:%d:" % (int(n), a.size) + a.tobytes())
    return h.hexdigest()


def encoder_tensors(text_encoder):
    """{name: tensor} of everything a frozen encoder computes from: its ``state_dict()`` and, for SBERT_ENCODER, the frozen tensors it keeps
    outside of it"""
    out = dict(text_encoder.state_dict())
    for k, v in getattr(text_encoder, "_w", {}).items():
        out[f"_w.{k}"] = v
    return out


def encoder_fingerprint(text_encoder):
    """sha256 (hex) over name, dtype, shape and bytes of `encoder_tensors`, in sorted name order"""
    h = hashlib.sha256()
    for name, t in sorted(encoder_tensors(text_encoder).items()):
        t = t.detach().cpu().contiguous()
        h.update(f"{name}|{t.dtype}|{tuple(t.shape)}|".encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


class CacheWriter:
    """Writes one split's two files: `add` takes the captions in order (their sentence rows and valid token rows), `finish` writes the
    sentence block and the index and renames the ``.part`` files into place."""

    def __init__(self, out_dir, split, n, emb_dim):
        if emb_dim < 4 or emb_dim % 4:
            raise ValueError(f"caption cache: emb_dim {emb_dim} is not a multiple of 4 (every row starts on a 16-byte boundary)")
        os.makedirs(out_dir, exist_ok=True)
        self.f32_path, self.idx_path = cache_paths(out_dir, split)
        self.split, self.n, self.e = split, int(n), int(emb_dim)
        self.sent = np.zeros((self.n, self.e), np.float32)
        self.lens = np.zeros(self.n, np.int32)
        self.done = 0
        self.f = open(self.f32_path + ".part", "wb")
        self.f.seek(self.n * self.e * 4)                       # the token rows come after the sentence block, which is written last

    def add(self, sent, tok, lens):
        """sent f32 [k, E], tok f32 [sum(lens), E] (caption by caption, valid tokens only), lens int [k]"""
        sent, tok, lens = np.asarray(sent, np.float32), np.ascontiguousarray(tok, np.float32), np.asarray(lens, np.int64)
        k = len(lens)
        if sent.shape != (k, self.e) or tok.shape != (int(lens.sum()), self.e) or (lens < 1).any() or self.done + k > self.n:
            raise ValueError(f"caption cache: {k} captions with sentence rows {sent.shape} and token rows {tok.shape} for lengths summing to "
                             f"{int(lens.sum())} at E = {self.e} ({self.done} of {self.n} written)")
        self.sent[self.done:self.done + k] = sent
        self.lens[self.done:self.done + k] = lens
        self.f.write(tok.tobytes())
        self.done += k

    def finish(self, keys, meta):
        if self.done != self.n or len(keys) != self.n:
            raise ValueError(f"caption cache: {self.done} captions written, {self.n} expected, {len(keys)} keys")
        self.f.seek(0)
        self.f.write(self.sent.tobytes())
        self.f.close()
        offsets = np.zeros(self.n, np.int64)
        offsets[1:] = np.cumsum(self.lens.astype(np.int64))[:-1]
        with open(self.idx_path + ".part", "wb") as f:
            np.savez(f, lens=self.lens, tok_offsets=offsets, keys=np.array([str(k) for k in keys], dtype=str), version=FORMAT_VERSION,
                     split=self.split, **meta)
        os.replace(self.f32_path + ".part", self.f32_path)
        os.replace(self.idx_path + ".part", self.idx_path)
        return self.f32_path, self.idx_path

    def abort(self):
        self.f.close()
        for p in (self.f32_path + ".part", self.idx_path + ".part"):
            if os.path.exists(p):
                os.remove(p)


def _collate(captions):
    """a batch of `handed_out_captions` entries as the DataLoader collates them"""
    lens = torch.tensor([int(n) for _, n in captions], dtype=torch.int64)
    if isinstance(captions[0][0], str):
        return [c for c, _ in captions], lens
    return torch.from_numpy(np.stack([np.asarray(c) for c, _ in captions]).astype(np.int64)), lens


def build_cache(cfg, data_dir, split, text_encoder, out_dir=None, batch_size=None, encoder_source=RANDOM_SOURCE):
    """Encode the handed-out caption of every image of ``split`` with ``text_encoder`` (frozen, on the GPU, in the engine's current
    precision) in batches of ``batch_size`` (default ``cfg.TRAIN.BATCH_SIZE``; the last batch filled up with captions already seen, see the
    module docstring) and write the two cache files into ``out_dir`` (default ``<data_dir>/caption_cache``).  ValueError, and nothing
    written, when a batch's outputs are not what the format relies on: a mask that is not a prefix, a value other than zero at t >= len."""
    from xmc_gan.dataset import SentTextDataset, WordTextDataset
    from . import ops
    if split not in ("train", "test"):
        raise ValueError(f"split {split!r}: 'train' or 'test'")
    arch = {"WORD": WordTextDataset, "SENT": SentTextDataset}[cfg.TEXT.TYPE]
    ds = arch(data_dir=data_dir, mode=split, transform=None, cfg=cfg)
    caps = handed_out_captions(ds)
    n, bs = len(caps), int(batch_size or cfg.TRAIN.BATCH_SIZE)
    if n < 1 or bs < 1:
        raise ValueError(f"caption cache: {n} captions, batch size {bs}")
    meta = cfg_meta(cfg)
    E, T = meta["emb_dim"], meta["max_length"]
    out_dir = out_dir or os.path.join(data_dir, "caption_cache")
    w = CacheWriter(out_dir, split, n, E)
    try:
        for s in range(0, n, bs):
            keep = min(bs, n - s)
            idx = list(range(s, s + keep)) + [j % n for j in range(bs - keep)]       # the filler: captions already seen
            c, l = _collate([caps[i] for i in idx])
            with torch.no_grad():
                words, sent, mask = text_encoder(c, l)
            if tuple(words.shape) != (bs, E, T) or tuple(sent.shape) != (bs, E) or tuple(mask.shape) != (bs, T) or words.dtype != torch.float32 \
                    or sent.dtype != torch.float32 or mask.dtype != torch.bool:
                raise ValueError(f"caption cache: the encoder returned {words.dtype} {tuple(words.shape)}, {sent.dtype} {tuple(sent.shape)}, "
                                 f"{mask.dtype} {tuple(mask.shape)}; f32 [{bs},{E},{T}], f32 [{bs},{E}], bool [{bs},{T}] expected")
            lens = (~mask).sum(1)
            prefix = torch.arange(T, device=mask.device)[None, :] >= lens[:, None]
            if not torch.equal(mask, prefix) or int(lens.min()) < 1:
                raise ValueError(f"caption cache: captions {s}..{s + keep - 1}: the encoder's mask is not `t >= len` with len >= 1 (a padding "
                                 "id inside a caption?); only the valid tokens can be stored")
            if bool((words.transpose(1, 2)[mask] != 0).any()):
                raise ValueError(f"caption cache: captions {s}..{s + keep - 1}: the encoder returned a non-zero value at t >= len; only the "
                                 "valid tokens can be stored")
            valid = ~mask
            valid[keep:] = False
            w.add(sent[:keep].cpu().numpy(), words.transpose(1, 2)[valid].cpu().numpy(), lens[:keep].cpu().numpy())
        return w.finish(ds.filenames, dict(meta, precision=ops.precision(), batch_size=bs, captions_fingerprint=captions_fingerprint(caps),
                                           encoder_fingerprint=encoder_fingerprint(text_encoder), encoder_source=str(encoder_source)))
    except BaseException:
        w.abort()
        raise


def construct_encoder(cfg, device, sbert_dir=None, proj_dir=None):
    """The frozen text encoder as ``train_gan.main`` constructs it: (encoder on ``device`` in eval mode, where its weights came from).  SBERT:
    the model directory ``sbert_dir`` / $XMC_SBERT_DIR; RNN: the state dict ``<proj_dir>/<TEXT.ENCODER_DIR>`` ('' leaves the initialisation)."""
    from xmc_gan.model.encoder import RNN_ENCODER, SBERT_ENCODER
    if cfg.TEXT.ENCODER_NAME == "SBERT":
        enc = SBERT_ENCODER(cfg=cfg, model_dir=sbert_dir or None).to(device).eval()
        return enc, enc.model_dir
    enc = RNN_ENCODER(cfg=cfg).to(device)
    source = RANDOM_SOURCE
    if cfg.TEXT.ENCODER_DIR != "":
        source = os.path.join(proj_dir or "", cfg.TEXT.ENCODER_DIR)
        enc.load_state_dict(torch.load(source, map_location=device))
    for p_ in enc.parameters():
        p_.requires_grad = False
    return enc.eval(), source


class CaptionCache:
    """The index of one split's cache and the path of its floats; `load` is the only way to get one, and it checks everything
    `CachedTextEncoder` and the kernel rely on."""

    def __init__(self, f32_path, lens, tok_offsets, keys, split, meta):
        self.f32_path, self.lens, self.tok_offsets, self.keys, self.split, self.meta = f32_path, lens, tok_offsets, keys, split, meta
        self.emb_dim, self.max_length = meta["emb_dim"], meta["max_length"]
        self.encoder, self.rnn_type = meta["encoder"], meta["rnn_type"]
        self.tok_rows = int(lens.astype(np.int64).sum())
        self.nfloats = (len(keys) + self.tok_rows) * self.emb_dim
        self.nbytes = self.nfloats * 4

    def __len__(self):
        return len(self.keys)

    def memmap(self):
        return np.memmap(self.f32_path, dtype=np.float32, mode="r", shape=(self.nfloats,))

    def entry(self, i):
        """(words_embs [E, max_length], sent_embs [E], mask [max_length]) of caption i as host arrays (copies): what the encoder returned"""
        E, T, n, o = self.emb_dim, self.max_length, int(self.lens[i]), int(self.tok_offsets[i])
        mm = self.memmap()
        words = np.zeros((E, T), np.float32)
        base = (len(self) + o) * E
        words[:, :n] = np.array(mm[base:base + n * E]).reshape(n, E).T
        return words, np.array(mm[i * E:(i + 1) * E]), np.arange(T) >= n

    def matches_encoder(self, text_encoder):
        """True when ``text_encoder`` holds the tensors the cache was built from (their names, dtypes, shapes and bytes)"""
        return encoder_fingerprint(text_encoder) == self.meta["encoder_fingerprint"]

    @classmethod
    def load(cls, cache_dir, split, cfg, text_dataset, precision, cfg_path="<yml>"):
        """The cache of ``split`` in ``cache_dir``, checked against ``cfg.TEXT``, the captions ``text_dataset`` (built with ``transform=None``)
        hands out and the run's ``precision``.  ValueError with the command that rebuilds it: files missing, another version / split, keys
        that are not ``text_dataset.filenames``, other captions, another emb_dim / max_length / encoder / rnn_type / bert_norm / pooling,
        another precision, offsets that do not increase by ``lens``, a file of the wrong length."""
        f32_path, idx_path = cache_paths(cache_dir, split)
        data_dir = getattr(text_dataset, "data_dir", "<data_dir>")
        how = f"; rebuild it with `{build_command(cfg_path, data_dir, split, cache_dir, precision)}`"

        def bad(msg):
            return ValueError(f"caption cache {idx_path}: {msg}{how}")
        for p in (f32_path, idx_path):
            if not os.path.isfile(p):
                raise ValueError(f"caption cache: {p} is missing{how}")
        names = ("lens", "tok_offsets", "keys", "version", "split", "precision", "batch_size", "captions_fingerprint", "encoder_fingerprint",
                 "encoder_source") + _META
        try:
            with np.load(idx_path, allow_pickle=False) as z:
                d = {k: z[k] for k in names}
        except (KeyError, OSError, ValueError) as e:
            raise bad(f"unreadable index ({type(e).__name__}: {e})")
        if int(d["version"]) != FORMAT_VERSION:
            raise bad(f"format version {int(d['version'])}, this code reads {FORMAT_VERSION}")
        if str(d["split"]) != split:
            raise bad(f"built for split {str(d['split'])!r}, not {split!r}")
        cached_keys = [str(k) for k in d["keys"]]
        if cached_keys != [str(k) for k in text_dataset.filenames]:
            raise bad(f"its {len(cached_keys)} keys are not the {len(text_dataset.filenames)} keys of {split}/filenames.pickle")
        meta = dict(emb_dim=int(d["emb_dim"]), max_length=int(d["max_length"]), encoder=str(d["encoder"]), rnn_type=str(d["rnn_type"]),
                    bert_norm=bool(d["bert_norm"]), pooling=str(d["pooling"]))
        want = cfg_meta(cfg)
        diff = [f"{k} {meta[k]!r} (the preset: {want[k]!r})" for k in _META if meta[k] != want[k]]
        if diff:
            raise bad("built with " + ", ".join(diff))
        if str(d["precision"]) != str(precision):
            raise bad(f"encoded in the {str(d['precision'])} mode, this run is in the {precision} mode")
        if captions_fingerprint(handed_out_captions(text_dataset)) != str(d["captions_fingerprint"]):
            raise bad("the captions the dataset hands out are not the captions it was built from (another captions fingerprint)")
        lens, off = d["lens"], d["tok_offsets"]
        n, E, T = len(cached_keys), meta["emb_dim"], meta["max_length"]
        if n < 1 or lens.dtype != np.int32 or off.dtype != np.int64 or not (lens.shape == off.shape == (n,)):
            raise bad("lens / tok_offsets are not int32 / int64 vectors of the keys' length")
        if E < 4 or E % 4 or not 1 <= T <= 64:
            raise bad(f"emb_dim {E} must be a multiple of 4 and max_length {T} in [1, 64]")
        if (lens < 1).any() or (lens > T).any() or off[0] != 0 or (off[1:] != off[:-1] + lens[:-1]).any():
            raise bad(f"lens are not in [1, {T}] or tok_offsets do not start at 0 and increase by lens")
        meta.update(precision=str(d["precision"]), batch_size=int(d["batch_size"]), captions_fingerprint=str(d["captions_fingerprint"]),
                    encoder_fingerprint=str(d["encoder_fingerprint"]), encoder_source=str(d["encoder_source"]))
        cache = cls(f32_path, lens, off, cached_keys, split, meta)
        if os.path.getsize(f32_path) != cache.nbytes:
            raise bad(f"{f32_path} has {os.path.getsize(f32_path)} bytes; {n} sentence rows and {cache.tok_rows} token rows of {E} floats are "
                      f"{cache.nbytes}")
        return cache


class CachedTextEncoder(torch.nn.Module):
    """Stands where the frozen text encoder stands in train_gan.py: ``forward_keys(keys)`` returns the ``(words_embs [B,E,T], sent_embs [B,E],
    mask [B,T])`` the encoder returned for those images' captions when ``cache`` (a `CaptionCache`) was built -- same shapes, dtypes and
    device, new tensors per call, one `ops.caption_gather` launch on the current stream.  No parameters.  The tables are uploaded here,
    once, through one pinned staging buffer in chunks of at most 256 MB.  ``reserve``: bytes of device memory that must stay free after
    the upload.  ``encoder_name`` / ``rnn_type`` / ``emb_dim``: of the encoder that built the cache.  ``eval_encoder``: the encoder of the
    test split when this one is the train split's (train() hands it to eval(); None: this one)."""

    def __init__(self, cache, device, reserve=DEFAULT_RESERVE):
        super().__init__()
        from . import ops
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("CachedTextEncoder keeps the tables on the GPU (no CPU fallback)")
        self._ops, self.cache, self.device = ops, cache, device
        self.encoder_name, self.rnn_type, self.emb_dim, self.max_length = cache.encoder, cache.rnn_type, cache.emb_dim, cache.max_length
        self.eval_encoder = None
        n, E = len(cache), cache.emb_dim
        free, _total = torch.cuda.mem_get_info(device)
        if cache.nbytes + reserve > free:
            raise RuntimeError(f"CachedTextEncoder: the {cache.split} tables of {cache.nbytes} bytes ({n * E * 4} of sentence rows, "
                               f"{cache.tok_rows * E * 4} of token rows) do not fit in the {free} bytes of free device memory with {reserve} "
                               f"bytes kept in reserve (tables in host memory are not supported)")
        self.table = torch.empty(cache.nfloats, dtype=torch.float32, device=device)
        mm = cache.memmap()
        chunk = min(UPLOAD_CHUNK // 4, cache.nfloats)
        staging = torch.empty(chunk, dtype=torch.float32).pin_memory()
        view = staging.numpy()
        for o in range(0, cache.nfloats, chunk):
            m = min(chunk, cache.nfloats - o)
            view[:m] = mm[o:o + m]
            self.table[o:o + m].copy_(staging[:m])             # (synchronous: the staging buffer is free again when it returns)
        del staging, view, mm
        self.sent_tab = self.table[:n * E].view(n, E)
        self.tok_tab = self.table[n * E:].view(cache.tok_rows, E)
        self.tok_offsets = torch.from_numpy(np.ascontiguousarray(cache.tok_offsets)).to(device)
        self.lens = torch.from_numpy(np.ascontiguousarray(cache.lens)).to(device)
        self._row_of = {k: i for i, k in enumerate(cache.keys)}

    def __len__(self):
        return len(self.cache)

    def train(self, mode=True):            # nothing to train: the module stays in eval mode, as the encoders it replaces
        return super().train(False)

    @torch.no_grad()
    def forward_rows(self, rows):
        """rows: a host int array [B] of caption rows (uploaded from pinned memory, without synchronising the device) or an `ops.HostMirror`
        of int32 [B].  ValueError, and nothing launched, for a row outside [0, N)."""
        ops = self._ops
        if not isinstance(rows, ops.HostMirror):
            if torch.is_tensor(rows):
                if rows.device.type != "cpu":
                    raise ValueError("CachedTextEncoder.forward_rows: rows must come with their host copy (a host array or an ops.HostMirror)")
                rows = rows.numpy()
            host = np.asarray(rows)
            if host.dtype.kind not in "iu":
                raise ValueError(f"CachedTextEncoder.forward_rows: integer rows expected, got {host.dtype}")
            if host.size and (host.min() < 0 or host.max() >= len(self)):      # (before the cast: an int64 row must not wrap into range)
                ops.validate_caption_rows(np.clip(host, -1, len(self)).astype(np.int32), len(self))
            host = np.ascontiguousarray(host, dtype=np.int32)
            ops.validate_caption_rows(host, len(self))
            dev = torch.from_numpy(host).pin_memory().to(self.device, non_blocking=True)
            rows = ops.HostMirror(host, dev=dev)
        return ops.caption_gather(self.sent_tab, self.tok_tab, self.tok_offsets, self.lens, rows, self.max_length)

    def forward_keys(self, keys):
        """keys: the loader's ``keys`` of a batch.  KeyError for a key that is not in the cache."""
        try:
            rows = np.fromiter((self._row_of[str(k)] for k in keys), dtype=np.int32, count=len(keys))
        except KeyError as e:
            raise KeyError(f"{e.args[0]!r} is not among the {len(self)} keys of the {self.cache.split} caption cache") from None
        return self.forward_rows(rows)

    def forward(self, caps=None, cap_lens=None, **kwargs):
        raise TypeError("CachedTextEncoder does not encode captions: call forward_keys(keys) with the loader's keys (the cache holds the "
                        "encoder's outputs for the one caption per image the datasets hand out)")
