"""Training batches from a device-resident uint8 image cache (``train_gan.py --image_cache DIR``).

The PIL path decodes and resizes every JPEG in every epoch.  Its deterministic part -- ``Image.open().convert('RGB')`` and the split's
``Resize`` of xmc_gan/dataset.py -- is done ONCE by `build_cache` and stored as raw RGB bytes; the random part (crop offset, flip) and the
normalisation are one kernel launch per batch over a pool that is uploaded once and stays in HBM (`ops.crop_flip_normalize`).

Format (version 1), two files per (split, size):

  ``<split>_<S>.u8``       the images' HWC bytes back to back in the order of ``<data_dir>/<split>/filenames.pickle``; every image starts on a
                           16-byte boundary, the file is a multiple of 16 bytes long and ends with at least 16 zero bytes after the last
                           image, so an aligned 16-byte load that covers the last pixel stays inside the buffer
  ``<split>_<S>.idx.npz``  ``offsets`` int64 [N], ``heights`` / ``widths`` int32 [N], ``keys`` [N], ``version``, ``split``, ``size``, ``resize``

train: ``Resize(int(S * 76 / 64))`` (shorter side, aspect kept: H x W varies per image); test: ``Resize((S, S))``.

Sampling (`DeviceImageLoader`, ``train=True``) is drawn on the host by numpy generators seeded from (seed, epoch) for the permutation -- the same
on every rank, rank r takes ``perm[r::world]`` as ``DistributedSampler(shuffle=True, drop_last=True)`` does -- and from (seed, rank, epoch) for
the crop offsets and flips.  The PIL path draws the same distributions from torch's global RNG inside each worker process, so the two paths
see the same distribution of batches, not the same batches.

Out of scope: pools that do not fit in device memory (no host streaming), per-rank shards of the pool (every rank holds all of it), writing
the engine's [N,H,W,8] layout directly.  (Cached caption embeddings: xmc_gan_amd/captioncache.py, ``--caption_cache``.)
"""
import collections
import os
import pickle
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

FORMAT_VERSION = 1
ALIGN = 16                         # every image's first byte, and the length of the file
TAIL = 16                          # zero bytes after the last image, at least
UPLOAD_CHUNK = 256 << 20           # bytes per host-to-device copy of the pool
DEFAULT_RESERVE = 8 << 30          # device memory the upload leaves free for the training step


def _usable_cores():
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 1
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, n)


def resize_rule(split, size):
    """(the split's deterministic transform of xmc_gan/dataset.py, its description as the index file records it)"""
    from xmc_gan.dataset import Resize
    if split == "train":
        t = int(size * 76 / 64)
        return Resize(t), f"shorter side -> {t}, bilinear"
    if split == "test":
        return Resize((size, size)), f"exact {size} x {size}, bilinear"
    raise ValueError(f"split {split!r}: 'train' or 'test'")


def cache_paths(cache_dir, split, size):
    stem = os.path.join(cache_dir, f"{split}_{int(size)}")
    return stem + ".u8", stem + ".idx.npz"


def build_command(data_dir, size, split, cache_dir):
    return f"python xmc_gan/image_cache.py build --data_dir {data_dir} --imsize {int(size)} --split {split} --out {cache_dir}"


def read_keys(data_dir, split):
    path = os.path.join(data_dir, split, "filenames.pickle")
    if not os.path.isfile(path):
        raise ValueError(f"{path} is missing")
    with open(path, "rb") as f:
        return [str(k) for k in pickle.load(f)]


def build_cache(data_dir, size, split, out_dir=None, threads=None):
    """Decode ``<data_dir>/images/<key>.jpg`` for every key of the split, apply the split's Resize and write the two cache files into
    ``out_dir`` (default ``<data_dir>/image_cache``).  Decoding runs in a pool of at most 16 threads (PIL releases the GIL while it decodes;
    default: min(16, usable cores)); the images are written in key order, a bounded number of them in flight.  Returns the two paths."""
    from PIL import Image
    size = int(size)
    transform, rule = resize_rule(split, size)
    keys = read_keys(data_dir, split)
    out_dir = out_dir or os.path.join(data_dir, "image_cache")
    os.makedirs(out_dir, exist_ok=True)
    threads = min(16, _usable_cores()) if threads is None else max(1, min(16, int(threads)))
    u8_path, idx_path = cache_paths(out_dir, split, size)

    def decode(key):
        with Image.open(os.path.join(data_dir, "images", f"{key}.jpg")) as im:
            a = np.array(transform(im.convert("RGB")), dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"{key}: decoded to {a.shape}, RGB expected")
        return a

    n = len(keys)
    offsets, heights, widths = np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int32)
    pos, done, submitted = 0, 0, 0
    pending = collections.deque()
    with open(u8_path + ".part", "wb") as f, ThreadPoolExecutor(threads) as ex:
        while done < n:
            while submitted < n and len(pending) < 4 * threads:
                pending.append(ex.submit(decode, keys[submitted]))
                submitted += 1
            a = pending.popleft().result()
            pad = (-pos) % ALIGN
            f.write(b"\0" * pad)
            pos += pad
            offsets[done], heights[done], widths[done] = pos, a.shape[0], a.shape[1]
            f.write(a.tobytes())
            pos += a.size
            done += 1
        f.write(b"\0" * ((-pos) % ALIGN + TAIL))
    os.replace(u8_path + ".part", u8_path)
    with open(idx_path, "wb") as f:
        np.savez(f, offsets=offsets, heights=heights, widths=widths, keys=np.array(keys, dtype=str), version=FORMAT_VERSION, split=split,
                 size=size, resize=rule)
    return u8_path, idx_path


class ImageCache:
    """The index of one (split, size) cache and the path of its bytes; `load` is the only way to get one, and it checks everything the
    loader and the kernel rely on."""

    def __init__(self, u8_path, offsets, heights, widths, keys, split, size, nbytes):
        self.u8_path, self.offsets, self.heights, self.widths = u8_path, offsets, heights, widths
        self.keys, self.split, self.size, self.nbytes = keys, split, size, nbytes

    def __len__(self):
        return len(self.keys)

    @property
    def hw(self):
        return np.ascontiguousarray(np.stack([self.heights, self.widths], 1).astype(np.int32))

    def memmap(self):
        return np.memmap(self.u8_path, dtype=np.uint8, mode="r", shape=(self.nbytes,))

    def image(self, i):
        """image i as a uint8 [H,W,3] array (a copy): what the PIL path would crop from"""
        h, w, o = int(self.heights[i]), int(self.widths[i]), int(self.offsets[i])
        return np.array(self.memmap()[o:o + h * w * 3]).reshape(h, w, 3)

    @classmethod
    def load(cls, cache_dir, split, size, keys, data_dir="<data_dir>"):
        """The cache of (split, size) in ``cache_dir``, checked against ``keys`` (the split's filenames.pickle, in order).  ValueError with
        the command that rebuilds it: files missing, another version / split / size, other keys, offsets that are not 16-byte aligned and
        increasing, images that overlap or end outside the file, a crop size that does not fit an image."""
        size = int(size)
        u8_path, idx_path = cache_paths(cache_dir, split, size)
        how = f"; rebuild it with `{build_command(data_dir, size, split, cache_dir)}`"

        def bad(msg):
            return ValueError(f"image cache {idx_path}: {msg}{how}")
        for p in (u8_path, idx_path):
            if not os.path.isfile(p):
                raise ValueError(f"image cache: {p} is missing{how}")
        try:
            with np.load(idx_path, allow_pickle=False) as z:
                d = {k: z[k] for k in ("offsets", "heights", "widths", "keys", "version", "split", "size", "resize")}
        except (KeyError, OSError, ValueError) as e:
            raise bad(f"unreadable index ({type(e).__name__}: {e})")
        if int(d["version"]) != FORMAT_VERSION:
            raise bad(f"format version {int(d['version'])}, this code reads {FORMAT_VERSION}")
        if str(d["split"]) != split or int(d["size"]) != size or str(d["resize"]) != resize_rule(split, size)[1]:
            raise bad(f"built for split {str(d['split'])!r} at size {int(d['size'])} ({str(d['resize'])}), not {split!r} at {size}")
        cached_keys = [str(k) for k in d["keys"]]
        if cached_keys != [str(k) for k in keys]:
            raise bad(f"its {len(cached_keys)} keys are not the {len(keys)} keys of {split}/filenames.pickle")
        off, hs, ws = d["offsets"], d["heights"], d["widths"]
        n = len(cached_keys)
        if n < 1 or off.dtype != np.int64 or hs.dtype != np.int32 or ws.dtype != np.int32 or not (off.shape == hs.shape == ws.shape == (n,)):
            raise bad("offsets / heights / widths are not int64 / int32 / int32 vectors of the keys' length")
        nbytes = os.path.getsize(u8_path)
        ends = off + hs.astype(np.int64) * ws.astype(np.int64) * 3
        if (hs < 1).any() or (ws < 1).any() or (off < 0).any() or (off % ALIGN).any() or (off[1:] < ends[:-1]).any():
            raise bad("offsets are not 16-byte aligned and increasing past each image")
        if nbytes % ALIGN or ends[-1] + TAIL > nbytes:
            raise bad(f"{u8_path} has {nbytes} bytes; the last image ends at {int(ends[-1])} and {TAIL} bytes of padding follow it")
        if (hs < size).any() or (ws < size).any():
            raise bad(f"an image is smaller than the {size} x {size} crop")
        return cls(u8_path, off, hs, ws, cached_keys, split, size, nbytes)


# ----------------------------------------------------------------------------------------------------------------- sampling (host only)
def epoch_indices(n, batch_size, seed, epoch, rank=0, world=1):
    """The image indices rank ``rank`` sees in epoch ``epoch``, int64 [batches, batch_size]: a permutation of range(n) from a generator
    seeded by (seed, epoch) -- the same on every rank --, of which the rank takes ``perm[rank::world]``, cut to n // world entries
    (DistributedSampler(shuffle=True, drop_last=True)'s partition) and then to whole batches (drop_last=True)."""
    perm = np.random.default_rng([int(seed), int(epoch)]).permutation(int(n))
    mine = perm[rank::world][:n // world]
    nb = len(mine) // batch_size
    return mine[:nb * batch_size].reshape(nb, batch_size).astype(np.int64)


def epoch_params(indices, hw, size, seed, epoch, rank=0):
    """int32 [batches, batch_size, 4] rows (index, top, left, flip) for `epoch_indices`' output: top uniform in [0, h - size], left uniform
    in [0, w - size], flip with p = 0.5, from a generator seeded by (seed, rank, epoch)"""
    rng = np.random.default_rng([int(seed), int(rank), int(epoch)])
    h, w = hw[indices, 0].astype(np.int64), hw[indices, 1].astype(np.int64)
    top, left = rng.integers(0, h - size + 1), rng.integers(0, w - size + 1)
    flip = rng.integers(0, 2, size=indices.shape)
    return np.ascontiguousarray(np.stack([indices, top, left, flip], -1).astype(np.int32))


def ordered_params(n, batch_size):
    """(indices, params) of the evaluation order: file order, whole batches, top = left = flip = 0"""
    nb = n // batch_size
    idx = np.arange(nb * batch_size, dtype=np.int64).reshape(nb, batch_size)
    p = np.zeros((nb, batch_size, 4), np.int32)
    p[..., 0] = idx
    return idx, p


# ----------------------------------------------------------------------------------------------------------------- the loader
class DeviceImageLoader:
    """Stands where ``torch.utils.data.DataLoader(TextDataset(...), batch_size, drop_last=True)`` stands in train_gan.py and yields the same
    ``(imgs, [(caps, cap_lens)], keys)`` -- with ``imgs`` an f32 [B,3,S,S] tensor made on the device by one `ops.crop_flip_normalize` launch
    on the current stream (a new tensor per batch), captions as the DataLoader collates them (WORD: LongTensor [B,T] and LongTensor [B];
    SENT: list of str and LongTensor [B]) and ``keys`` a list of str.

    ``cache``: an `ImageCache`; its bytes are uploaded here, once, through one pinned staging buffer in chunks of at most 256 MB.
    ``text_dataset``: a WordTextDataset / SentTextDataset built with ``transform=None``; only its captions (the fixed ``sent_ix = 1`` of
    ``TextDataset.__getitem__``, gathered here once) and filenames are used -- no image is opened.
    ``train=True``: `epoch_indices` / `epoch_params` with epoch = start_epoch + 1, + 2, ... per ``__iter__``; ``train=False``: file order,
    top = left = flip = 0.  ``last_params``: (indices int64 [B], params int32 [B,4]) of the batch yielded last.
    ``reserve``: bytes of device memory that must stay free after the upload (the training step's)."""

    def __init__(self, cache, text_dataset, batch_size, device, train, seed=0, rank=0, world=1, start_epoch=0, reserve=DEFAULT_RESERVE):
        from . import ops
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("DeviceImageLoader keeps the images on the GPU (no CPU fallback)")
        n = len(cache)
        if [str(k) for k in text_dataset.filenames] != cache.keys:
            raise ValueError("DeviceImageLoader: the cache's keys are not the text dataset's filenames")
        if getattr(text_dataset, "b_local", False):
            raise ValueError("DeviceImageLoader: b_local (a second, random caption per image) is not supported")
        if not 0 <= rank < world or batch_size < 1:
            raise ValueError(f"DeviceImageLoader: rank {rank} of {world}, batch size {batch_size}")
        self.cache, self.dataset, self.batch_size, self.device, self.train = cache, text_dataset, int(batch_size), device, bool(train)
        self.seed, self.rank, self.world, self.epoch = int(seed), int(rank), int(world), int(start_epoch)
        self.size, self.drop_last, self.last_params = cache.size, True, None
        self._ops = ops
        # captions: the one caption per image the PIL path's __getitem__ hands out
        per = text_dataset.caps_per_image
        caps = [text_dataset.get_caption(i * per + 1) for i in range(n)]
        self._lens = torch.tensor([c[1] for c in caps], dtype=torch.int64)
        self._word = not isinstance(caps[0][0], str)
        self._caps = torch.from_numpy(np.stack([c[0] for c in caps]).astype(np.int64)) if self._word else [c[0] for c in caps]
        # the pool, once
        free, _total = torch.cuda.mem_get_info(device)
        if cache.nbytes + reserve > free:
            raise RuntimeError(f"DeviceImageLoader: the {cache.split} pool of {cache.nbytes} bytes does not fit in the {free} bytes of free device "
                               f"memory with {reserve} bytes kept in reserve (streaming from host memory is not supported)")
        self.pool = torch.empty(cache.nbytes, dtype=torch.uint8, device=device)
        mm = cache.memmap()
        chunk = min(UPLOAD_CHUNK, cache.nbytes)
        staging = torch.empty(chunk, dtype=torch.uint8).pin_memory()
        view = staging.numpy()
        for o in range(0, cache.nbytes, chunk):
            m = min(chunk, cache.nbytes - o)
            view[:m] = mm[o:o + m]
            self.pool[o:o + m].copy_(staging[:m])              # (synchronous: the staging buffer is free again when it returns)
        del staging, view, mm
        self.offsets = torch.from_numpy(np.ascontiguousarray(cache.offsets)).to(device)
        self.hw = ops.HostMirror(cache.hw, device)
        self.table = ops.normalize_table(device)

    def _local(self):
        return len(self.cache) // self.world if self.train else len(self.cache)

    def __len__(self):
        return self._local() // self.batch_size

    def __iter__(self):
        if self.train:
            self.epoch += 1
            idx = epoch_indices(len(self.cache), self.batch_size, self.seed, self.epoch, self.rank, self.world)
            params = epoch_params(idx, self.hw.host, self.size, self.seed, self.epoch, self.rank)
        else:
            idx, params = ordered_params(len(self.cache), self.batch_size)
        if not len(idx):
            return
        dev = torch.from_numpy(params).to(self.device)           # the epoch's rows in one upload; a batch is a slice of it
        for b in range(len(idx)):
            rows = self._ops.HostMirror(params[b], dev=dev[b])
            imgs = self._ops.crop_flip_normalize(self.pool, self.offsets, self.hw, rows, self.size, table=self.table)
            ib = idx[b]
            caps = self._caps[torch.from_numpy(ib)] if self._word else [self._caps[i] for i in ib]
            self.last_params = (ib.copy(), params[b].copy())
            yield imgs, [(caps, self._lens[torch.from_numpy(ib)])], [self.cache.keys[i] for i in ib]
