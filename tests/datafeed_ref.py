"""Host restatement of the image-cache path, for tests/test_imagecache_*.py: the PIL operations of xmc_gan/dataset.py applied to the cached
bytes with GIVEN (top, left, flip) -- `Image.crop`, `transpose(FLIP_LEFT_RIGHT)`, `to_normalized_tensor` -- and a miniature COCO-layout tree
of generated JPEGs whose sizes exercise every branch of `Resize` and every byte alignment of the kernel."""
import pickle

import numpy as np
import torch
from PIL import Image

from xmc_gan.dataset import Resize, to_normalized_tensor


def crop_flip_normalize_ref(image_u8, top, left, flip, size):
    """uint8 [H,W,3] -> f32 [3,size,size] as RandomCrop / RandomHorizontalFlip / to_normalized_tensor do it once their draws are fixed"""
    img = Image.fromarray(np.ascontiguousarray(image_u8))
    img = img.crop((int(left), int(top), int(left) + size, int(top) + size))
    if flip:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    return to_normalized_tensor(img)


def batch_ref(images, params, size):
    """images: list of uint8 [H,W,3] (the cache's); params int [B,4] rows (index, top, left, flip) -> f32 [B,3,size,size]"""
    return torch.stack([crop_flip_normalize_ref(images[int(i)], t, l, f, size) for i, t, l, f in np.asarray(params)])


def resized_by_hand(path, split, size):
    """the bytes the cache must hold for one JPEG: the split's Resize of xmc_gan/dataset.py on the decoded RGB image"""
    t = Resize(int(size * 76 / 64)) if split == "train" else Resize((size, size))
    return np.array(t(Image.open(path).convert("RGB")), dtype=np.uint8)


def mini_tree(root, sizes, seed=1, sent=False, caps_per_image=5, max_words=12, voca=40):
    """images/<key>.jpg of the given (width, height) sizes with smooth random content, {train,test}/filenames.pickle, captions.pickle and
    (``sent``) bert_captions.pickle.  Returns (data_dir, keys)."""
    rng = np.random.RandomState(seed)
    (root / "images").mkdir(parents=True)
    keys = [f"k{i:03d}" for i in range(len(sizes))]
    for k, (w, h) in zip(keys, sizes):
        small = rng.randint(0, 256, ((h + 7) // 8, (w + 7) // 8, 3), dtype=np.uint8)
        Image.fromarray(small).resize((w, h), Image.BILINEAR).save(root / "images" / f"{k}.jpg", quality=92)
    for mode in ("train", "test"):
        (root / mode).mkdir()
        with open(root / mode / "filenames.pickle", "wb") as f:
            pickle.dump(keys, f)
    caps = [list(rng.randint(1, voca, size=rng.randint(2, max_words))) for _ in range(len(sizes) * caps_per_image)]
    i2w = {i: f"w{i}" for i in range(voca)}
    with open(root / "captions.pickle", "wb") as f:
        pickle.dump([caps, caps, i2w, {v: k for k, v in i2w.items()}], f)
    if sent:
        sents = [" ".join(i2w[t] for t in c) for c in caps]
        with open(root / "bert_captions.pickle", "wb") as f:
            pickle.dump([sents, sents], f)
    return str(root), keys
