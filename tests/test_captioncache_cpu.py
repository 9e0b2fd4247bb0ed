"""The caption-embedding cache without a GPU: the file format written and reloaded, every refusal of `CaptionCache.load` with the command that
rebuilds the cache, the captions fingerprint, the host-side bounds check of `ops.caption_gather`, and the C ABI of `xmc_caption_gather`."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]

import caption_ref as R  # noqa: E402
from xmc_gan_amd import captioncache as CC  # noqa: E402

E, T, N = 8, 5, 7
KEYS = [f"k{i:03d}" for i in range(N)]
LENS = R.kernel_lens(T)
BUILD = "python xmc_gan/caption_cache.py build"


@pytest.fixture()
def made(tmp_path):
    cfg = R.text_cfg(E, T)
    ds = R.ListTextDataset(KEYS, R.word_captions(N, T))
    out = str(tmp_path / "cache")
    sent, tok, off = R.write_cache(out, "train", KEYS, LENS, cfg, ds)
    return dict(out=out, cfg=cfg, ds=ds, sent=sent, tok=tok, off=off, paths=CC.cache_paths(out, "train"))


def test_a_written_cache_reloads_with_every_value(made):
    c = CC.CaptionCache.load(made["out"], "train", made["cfg"], made["ds"], "bf16")
    assert len(c) == N and c.keys == KEYS and c.emb_dim == E and c.max_length == T and c.encoder == "RNN" and c.rnn_type == "LSTM"
    assert c.lens.dtype == np.int32 and np.array_equal(c.lens, LENS) and c.tok_offsets.dtype == np.int64 and np.array_equal(c.tok_offsets, made["off"])
    assert c.tok_rows == int(LENS.sum()) and c.nbytes == (N + c.tok_rows) * E * 4 == os.path.getsize(made["paths"][0])
    assert c.meta["precision"] == "bf16" and c.meta["batch_size"] == 4 and c.meta["encoder_source"] == "hand-made"
    raw = np.fromfile(made["paths"][0], dtype=np.float32)
    assert np.array_equal(raw[:N * E].reshape(N, E), made["sent"]) and np.array_equal(raw[N * E:].reshape(-1, E), made["tok"])
    words, sent, mask = R.gather_ref(made["sent"], made["tok"], made["off"], LENS, range(N), T)
    for i in range(N):
        w, s, m = c.entry(i)
        assert np.array_equal(w, words[i]) and np.array_equal(s, sent[i]) and np.array_equal(m, mask[i])
    assert not [f for f in os.listdir(made["out"]) if f.endswith(".part")]


def _refused(made, match, split="train", cfg=None, ds=None, precision="bf16"):
    with pytest.raises(ValueError, match=match) as e:
        CC.CaptionCache.load(made["out"], split, cfg or made["cfg"], ds or made["ds"], precision, cfg_path="my.yml")
    msg = str(e.value)
    assert msg.endswith("`") and f"{BUILD} --cfg my.yml --data_dir DATA --split {split} --out {made['out']}" in msg, msg
    return msg


def test_load_refuses_missing_files(made, tmp_path):
    os.remove(made["paths"][0])
    _refused(made, "is missing")
    made2 = dict(made, out=str(tmp_path / "nothing"))
    _refused(made2, "is missing")


def test_load_refuses_another_version_and_another_split(made):
    f32, idx = made["paths"]
    for p in (f32, idx):                                              # the train files under the test split's names
        os.replace(p, p.replace("train.cap", "test.cap"))
    _refused(made, "built for split 'train'", split="test")
    R.rewrite_index(idx.replace("train.cap", "test.cap"), version=np.array(CC.FORMAT_VERSION + 1))
    _refused(made, "format version 2", split="test")


def test_load_refuses_other_keys_and_other_captions(made):
    other = R.ListTextDataset(KEYS[:-1] + ["zzz"], made["ds"].captions)
    _refused(made, "keys are not", ds=other)
    caps = list(made["ds"].captions)
    caps[3 * 5 + 1] = np.roll(caps[3 * 5 + 1], 1) + 1                 # the caption image 3 hands out
    _refused(made, "captions fingerprint", ds=R.ListTextDataset(KEYS, caps))


@pytest.mark.parametrize("field,cfg", [("emb_dim", R.text_cfg(12, T)), ("max_length", R.text_cfg(E, T + 1)), ("encoder", R.text_cfg(E, T, encoder="SBERT")),
                                       ("rnn_type", R.text_cfg(E, T, rnn_type="GRU"))])
def test_load_refuses_a_cache_of_another_text_configuration(made, field, cfg):
    assert field in _refused(made, "built with", cfg=cfg)


@pytest.mark.parametrize("field,cfg", [("bert_norm", R.text_cfg(E, T, encoder="SBERT", bert_norm=True)),
                                       ("pooling", R.text_cfg(E, T, encoder="SBERT", pooling="CLS"))])
def test_load_refuses_another_sbert_tail(tmp_path, field, cfg):
    built = R.text_cfg(E, T, encoder="SBERT")
    ds = R.ListTextDataset(KEYS, [f"w{i} w{i + 1}" for i in range(N * 5)])
    out = str(tmp_path / "cache")
    R.write_cache(out, "train", KEYS, LENS, built, ds)
    made = dict(out=out, cfg=built, ds=ds)
    CC.CaptionCache.load(out, "train", built, ds, "bf16")
    msg = _refused(made, "built with", cfg=cfg)
    assert field in msg and "emb_dim" not in msg.split("; rebuild")[0]


def test_load_refuses_another_precision(made):
    msg = _refused(made, "bf16 mode, this run is in the fp32 mode", precision="fp32")
    assert msg.endswith("--precision fp32`")


def test_load_refuses_offsets_that_do_not_increase_by_lens_and_a_short_file(made):
    f32, idx = made["paths"]
    off = made["off"].copy()
    off[4] += 1
    R.rewrite_index(idx, tok_offsets=off)
    _refused(made, "increase by lens")
    lens = LENS.copy()
    lens[1] = T + 1                                                   # a caption longer than the words tensor
    R.rewrite_index(idx, tok_offsets=made["off"], lens=lens)
    _refused(made, "increase by lens")
    R.rewrite_index(idx, tok_offsets=made["off"], lens=LENS)
    CC.CaptionCache.load(made["out"], "train", made["cfg"], made["ds"], "bf16")
    with open(f32, "ab") as f:
        f.write(b"\0" * 4)
    _refused(made, "bytes")
    with open(f32, "r+b") as f:
        f.truncate((N + int(LENS.sum())) * E * 4 - E * 4)
    _refused(made, "bytes")


def test_writer_refuses_a_width_that_is_no_multiple_of_4(tmp_path):
    with pytest.raises(ValueError, match="multiple of 4"):
        CC.CacheWriter(str(tmp_path), "train", 3, 6)


def test_captions_fingerprint_follows_the_handed_out_captions_only():
    per = 5
    caps = R.word_captions(N, T, per)
    fp = CC.captions_fingerprint(CC.handed_out_captions(R.ListTextDataset(KEYS, caps, per)))
    assert re.fullmatch(r"[0-9a-f]{64}", fp)
    others = [c if i % per == 1 else np.roll(c, 1) + 1 for i, c in enumerate(caps)]          # every caption that is NOT handed out
    assert CC.captions_fingerprint(CC.handed_out_captions(R.ListTextDataset(KEYS, others, per))) == fp
    for i in (0, N - 1):
        one = list(caps)
        one[i * per + 1] = caps[i * per + 1] + (caps[i * per + 1] > 0)                       # one token id of one handed-out caption
        assert CC.captions_fingerprint(CC.handed_out_captions(R.ListTextDataset(KEYS, one, per))) != fp
    sents = [f"a w{i}" for i in range(N * per)]
    fs = CC.captions_fingerprint(CC.handed_out_captions(R.ListTextDataset(KEYS, sents, per)))
    sents[1] = "a  w1"
    assert CC.captions_fingerprint(CC.handed_out_captions(R.ListTextDataset(KEYS, sents, per))) != fs != fp


def test_encoder_fingerprint_follows_names_and_bytes():
    a, b = torch.nn.Linear(3, 2), torch.nn.Linear(3, 2)
    b.load_state_dict(a.state_dict())
    assert CC.encoder_fingerprint(a) == CC.encoder_fingerprint(b)
    with torch.no_grad():
        b.weight[1, 2] += 1e-3
    assert CC.encoder_fingerprint(a) != CC.encoder_fingerprint(b)
    a._w = {"extra": torch.zeros(2)}                                  # tensors a frozen encoder keeps outside its state dict count too
    c = torch.nn.Linear(3, 2)
    c.load_state_dict(a.state_dict())
    assert CC.encoder_fingerprint(a) != CC.encoder_fingerprint(c)


# ------------------------------------------------------------------------------------------ the op's host side
def test_bad_rows_raise_before_any_library_call(monkeypatch):
    from xmc_gan_amd import ops
    import xmc_gan_amd.lib as L
    calls = []
    monkeypatch.setattr(L, "call", lambda name, *a: calls.append(name))
    monkeypatch.setattr(L, "load", lambda *a: calls.append("load"))
    sent, tok, off = R.tables(LENS, E)
    args = [torch.from_numpy(x) for x in (sent, tok, off, LENS)]
    for rows in ([0, -1, 2], [0, 1, N]):
        bad = np.array(rows, np.int32)
        with pytest.raises(ValueError, match="entry [12] = "):
            ops.caption_gather(*args, bad, T)
        with pytest.raises(ValueError, match="entry [12] = "):
            ops.caption_gather(*args, ops.HostMirror(bad, "cpu"), T)
        with pytest.raises(ValueError, match="entry [12] = "):
            ops.validate_caption_rows(bad, N)
    with pytest.raises(ValueError, match="host copy"):               # rows that exist on a device only cannot be checked without a read-back
        ops.caption_gather(*args, torch.empty(3, dtype=torch.int32, device="meta"), T)
    for wrong in (np.array([0, 1], np.int64), np.zeros((2, 1), np.int32), np.zeros(0, np.int32)):
        with pytest.raises(ValueError):
            ops.validate_caption_rows(wrong, N)
    ops.validate_caption_rows(np.array([0, N - 1, 0], np.int32), N)
    assert calls == []


def test_cached_encoder_does_not_encode_and_synthetic_excludes_the_flag():
    enc = CC.CachedTextEncoder.__new__(CC.CachedTextEncoder)
    with pytest.raises(TypeError, match="forward_keys"):
        CC.CachedTextEncoder.forward(enc, ["a caption"], torch.tensor([2]))
    import xmc_gan.train_gan as tg
    assert tg.parse_args([]).caption_cache == ""
    with pytest.raises(SystemExit, match="--caption_cache and --synthetic"):
        tg.main(["--caption_cache", "somewhere", "--synthetic", "2"])


def test_rprecision_accepts_a_cache_built_by_an_rnn_encoder_of_the_image_encoders_width():
    import types
    from xmc_gan_amd import rprecision as RP
    enc = CC.CachedTextEncoder.__new__(CC.CachedTextEncoder)
    torch.nn.Module.__init__(enc)
    image_encoder = types.SimpleNamespace(nef=256)
    enc.encoder_name, enc.rnn_type, enc.emb_dim = "RNN", "LSTM", 256
    assert RP.usable_with(enc, image_encoder) is None
    enc.emb_dim = 128
    assert "nef" in RP.usable_with(enc, image_encoder)
    enc.encoder_name, enc.emb_dim = "SBERT", 256
    assert "SBERT" in RP.usable_with(enc, image_encoder)


# ------------------------------------------------------------------------------------------ the C ABI, without a GPU
def test_header_binding_makefile_and_ops_agree_on_the_entry_point():
    import xmc_gan_amd.lib as L
    from xmc_gan_amd import ops
    hdr = open(os.path.join(ROOT, "include", "xmc_gan_hip.h")).read()
    m = re.search(r"\bint\s+xmc_caption_gather\s*\(([^)]*)\)\s*;", hdr)
    assert m, "no prototype"
    params = [p.strip() for p in m.group(1).split(",")]
    sig = L._SIGS["xmc_caption_gather"]
    assert len(params) == len(sig) == 14
    for p, c in zip(params, sig):                                     # pointers as void*, the 64-bit count as int64, the rest as int32
        want = L.vp if "*" in p else (L.i64 if p.startswith("int64_t") else L.i32)
        assert c is want, (p, c)
    note = hdr[hdr.index("Added without a new version"):hdr.index("#define XMC_ABI_VERSION")]
    assert "xmc_caption_gather" in note and "captionfeed.hip" in note
    mk = open(os.path.join(ROOT, "xmc-gan_amd", "csrc", "Makefile")).read()
    assert "captionfeed.hip" in mk[mk.index("SRCS"):mk.index("OBJS")]
    assert "xmc_caption_gather" in L.EXPORTS and callable(ops.caption_gather) and callable(ops.validate_caption_rows)
    src = open(os.path.join(ROOT, "xmc-gan_amd", "csrc", "captionfeed.hip")).read()
    assert "atomic" not in src.replace("No atomics", "") and "asm" not in src.replace("no inline assembly", "")
    assert 'xmc_note_kernel("caption_gather_kernel")' in src


def test_the_abi_version_is_13():
    import xmc_gan_amd.lib as L
    hdr = open(os.path.join(ROOT, "include", "xmc_gan_hip.h")).read()
    assert re.search(r"#define XMC_ABI_VERSION (\d+)", hdr).group(1) == "13" and L.ABI_VERSION == 13
    for variant in ("bf16", "f16"):
        assert L.load(variant).xmc_abi_version() == 13


@pytest.mark.parametrize("variant", ["bf16", "f16"])
def test_both_builds_refuse_bad_arguments_before_any_launch(variant):
    """a NULL pointer, N < 1, tok_rows < 1 -> XMC_EINVAL; B < 1, E < 4, E % 4 != 0, T < 1, T > 64 -> XMC_ESHAPE; a misaligned table, output or
    offsets vector -> XMC_EALIGN.  None of these calls launches, so this runs without a GPU."""
    import xmc_gan_amd.lib as L
    f = L.load(variant).xmc_caption_gather
    EINVAL, EALIGN, ESHAPE = -1, -2, -3
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 4)
    good = [p, p, 9, p, p, 3, p, 2, 8, 5, p, p, p, None]      # sent_tab, tok_tab, tok_rows, tok_offsets, lens, N, rows, B, E, T, words, sent, mask, stream

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return f(*a)
    for i in (0, 1, 3, 4, 6, 10, 11, 12):
        assert call(**{f"a{i}": None}) == EINVAL
    assert call(a5=0) == EINVAL and call(a2=0) == EINVAL
    assert call(a7=0) == ESHAPE and call(a8=6) == ESHAPE and call(a8=0) == ESHAPE and call(a8=2) == ESHAPE
    assert call(a9=0) == ESHAPE and call(a9=65) == ESHAPE and call(a9=-1) == ESHAPE
    for i in (0, 1, 3, 10, 11):
        assert call(**{f"a{i}": odd}) == EALIGN
