"""Host helpers for tests/test_captioncache_*.py (a helper, not a test): the numpy restatement of `ops.caption_gather` -- the copy and the
transposition, nothing else --, hand-made tables and caches in the format of xmc_gan_amd/captioncache.py, a text dataset without files, and
the shrunken DAMSM preset the entry-point tests run."""
import os
import types

import numpy as np

from golden_util import CFG_DIR


def kernel_lens(T):
    """the seven captions of the kernel tests: the shortest, the longest, and lengths in between"""
    return np.array([1, T, min(3, T), T - 1 if T > 1 else 1, min(2, T), T, 1], np.int32)


def tables(lens, E, seed=0):
    """(sent_tab f32 [N,E], tok_tab f32 [sum(lens),E], tok_offsets int64 [N]) of distinct, non-zero values"""
    rng = np.random.RandomState(seed)
    lens = np.asarray(lens, np.int32)
    n, rows = len(lens), int(lens.sum())
    sent = (rng.standard_normal((n, E)) + 3.0).astype(np.float32)
    tok = (np.arange(rows * E, dtype=np.float32).reshape(rows, E) + 1.0) * np.float32(0.25)        # every element its own value
    off = np.zeros(n, np.int64)
    off[1:] = np.cumsum(lens.astype(np.int64))[:-1]
    return sent, tok, off


def gather_ref(sent_tab, tok_tab, tok_offsets, lens, rows, T):
    """words f32 [B,E,T] (zero from len on), sent f32 [B,E], mask bool [B,T] (True at padding)"""
    B, E = len(rows), sent_tab.shape[1]
    words, sent, mask = np.zeros((B, E, T), np.float32), np.zeros((B, E), np.float32), np.ones((B, T), bool)
    for b, r in enumerate(rows):
        n, o = int(lens[r]), int(tok_offsets[r])
        words[b, :, :n] = tok_tab[o:o + n].T
        sent[b] = sent_tab[r]
        mask[b, :n] = False
    return words, sent, mask


def text_cfg(emb_dim=8, max_length=5, encoder="RNN", rnn_type="LSTM", bert_norm=False, pooling="MEAN", per=5):
    """the part of the experiment configuration a caption cache looks at"""
    return types.SimpleNamespace(TEXT=types.SimpleNamespace(EMBEDDING_DIM=emb_dim, MAX_LENGTH=max_length, ENCODER_NAME=encoder, RNN_TYPE=rnn_type,
                                                            BERT_NORM=bert_norm, POOLING_MODE=pooling, CAPTIONS_PER_IMAGE=per))


class ListTextDataset:
    """what `CaptionCache.load` and the builder read of a TextDataset: filenames, caps_per_image, data_dir and get_caption"""

    def __init__(self, keys, captions, per=5, data_dir="DATA"):
        assert len(captions) == len(keys) * per
        self.filenames, self.captions, self.caps_per_image, self.data_dir = list(keys), list(captions), per, data_dir

    def get_caption(self, ix):
        c = self.captions[ix]
        return (c, len(c.split(" "))) if isinstance(c, str) else (np.asarray(c, np.int64), int(np.count_nonzero(c)))


def word_captions(n_images, max_length, per=5, seed=2):
    rng = np.random.RandomState(seed)
    caps = []
    for _ in range(n_images * per):
        k = rng.randint(1, max_length + 1)
        c = np.zeros(max_length, np.int64)
        c[:k] = rng.randint(1, 40, size=k)
        caps.append(c)
    return caps


def write_cache(out_dir, split, keys, lens, cfg, dataset, precision="bf16", seed=0, **over):
    """a cache of hand-made values through `CacheWriter`, with the index fields the builder writes (``over`` replaces some).  Returns
    (sent_tab, tok_tab, tok_offsets)."""
    from xmc_gan_amd import captioncache as CC
    meta = CC.cfg_meta(cfg)
    sent, tok, off = tables(lens, meta["emb_dim"], seed)
    w = CC.CacheWriter(out_dir, split, len(keys), meta["emb_dim"])
    half = len(keys) // 2                                           # in two parts, as the builder adds batch after batch
    for a, b in ((0, half), (half, len(keys))):
        if b > a:
            w.add(sent[a:b], tok[int(off[a]):int(off[b - 1]) + int(lens[b - 1])], lens[a:b])
    fields = dict(meta, precision=precision, batch_size=4, captions_fingerprint=CC.captions_fingerprint(CC.handed_out_captions(dataset)),
                  encoder_fingerprint="0" * 64, encoder_source="hand-made")
    fields.update(over)
    w.finish(keys, fields)
    return sent, tok, off


def rewrite_index(idx_path, **fields):
    """the index file with some fields replaced"""
    with np.load(idx_path, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    d.update(fields)
    with open(idx_path, "wb") as f:
        np.savez(f, **d)


def mini_yml(tmp_path, name="mini.yml", **subst):
    """df_gan_damsm.yml shrunk for a test run (thin network, tiny vocabulary, no pretrained encoder file, MAX_LENGTH 8)"""
    txt = open(os.path.join(CFG_DIR, "df_gan_damsm.yml")).read()
    rep = {"NCH: 32": "NCH: 8", "VOCA_SIZE: 27297": "VOCA_SIZE: 40", "BATCH_SIZE: 88": "BATCH_SIZE: 4", "LOG_INTERVAL: 200": "LOG_INTERVAL: 2",
           "NUM_WORKERS: 8": "NUM_WORKERS: 0", "ENCODER_DIR: data/DAMSMencoders/coco/text_encoder100.pth": "ENCODER_DIR: ''",
           "MAX_LENGTH: 20": "MAX_LENGTH: 8", "MAGP: true": "MAGP: false"}
    rep.update(subst)
    for a, b in rep.items():
        assert a in txt, a
        txt = txt.replace(a, b)
    path = tmp_path / name
    path.write_text(txt)
    return str(path)
