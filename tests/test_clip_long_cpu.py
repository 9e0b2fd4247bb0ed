"""CPU-only checks of CLIPScore past 64 tokens (`CLIPScorer(..., max_tokens=N)`, `ops.attention_long`, csrc/attention_long.hip's C ABI and
the ``--clip_max_tokens`` wiring): what the loader accepts and refuses, the context and the truncation at CLIP's own 77 positions, the flag on
the three command lines, the entry point's declarations and its argument checks."""
import ctypes
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ref as R
import xmc_gan_amd.lib as L
from xmc_gan_amd import evaluate as EV
from xmc_gan_amd import ops
from xmc_gan_amd.clip import CLIPScorer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ the loader
def test_loader_takes_b16_and_l14_token_counts(tmp_path):
    """the sizes only: one narrow layer per tower at 224 / 16 (197 tokens) and 224 / 14 (257 tokens, a patch row of 588 columns)"""
    small = dict(width=64, layers=1, heads=1, ffn=64)
    R.write_model_dir(tmp_path / "b16", 1, R.hf_config(image=224, patch=16, **small))
    R.write_model_dir(tmp_path / "l14", 1, R.hf_config(image=224, patch=14, **small))
    b16, l14 = CLIPScorer(str(tmp_path / "b16"), max_tokens=257), CLIPScorer(str(tmp_path / "l14"), None, 257)
    assert (b16.tokens, b16.grid, l14.tokens, l14.grid) == (197, 14, 257, 16) and b16.max_tokens == l14.max_tokens == 257
    assert tuple(l14._w["v.patch"].shape) == (64, 588) and l14.g_patch.cin == 588
    assert (b16.vision.long, b16.text.long, b16.context) == (True, False, 24)                    # one kernel per tower, by its longest sequence
    assert CLIPScorer(str(tmp_path / "b16"), max_tokens=197).tokens == 197
    with pytest.raises(NotImplementedError) as e:
        CLIPScorer(str(tmp_path / "l14"), max_tokens=197)
    assert all(s in str(e.value) for s in ("257", "197", "--clip_max_tokens"))
    for name in ("b16", "l14"):                                                                  # without the argument: refused as before
        with pytest.raises(NotImplementedError, match="at most 64 tokens"):
            CLIPScorer(str(tmp_path / name))
        with pytest.raises(NotImplementedError, match="at most 64 tokens"):
            CLIPScorer(str(tmp_path / name), None, 64)
    for bad in (63, 1025, 0, -1, 77.0, None, True):
        with pytest.raises(ValueError, match="max_tokens"):
            CLIPScorer(str(tmp_path / "b16"), max_tokens=bad)
    # what stays refused whatever max_tokens says
    R.write_model_dir(tmp_path / "wide", 1, R.hf_config(width=1088, heads=17, layers=1))
    with pytest.raises(NotImplementedError, match="<= 1024"):
        CLIPScorer(str(tmp_path / "wide"), max_tokens=1024)
    R.write_model_dir(tmp_path / "d32", 1, R.hf_config(width=128, heads=4, layers=1))
    with pytest.raises(NotImplementedError, match="head dimension 64"):
        CLIPScorer(str(tmp_path / "d32"), max_tokens=1024)


def test_context_and_truncation_follow_clip_at_77(tmp_path):
    tk = pytest.importorskip("tokenizers")
    words = [f"w{i}" for i in range(40)]
    hf = R.hf_config(vocab=60, max_pos=77, layers=1)
    R.write_model_dir(tmp_path / "m", 3, hf, tokenizer=R.word_tokenizer(words))
    d = str(tmp_path / "m")
    default, opted = CLIPScorer(d), CLIPScorer(d, max_tokens=128)
    assert (default.context, default.vision.long, default.text.long) == (64, False, False)      # today's scorer
    assert (opted.context, opted.tokens, opted.vision.long, opted.text.long) == (77, 17, False, True)
    assert CLIPScorer(d, max_tokens=77).context == 77 and CLIPScorer(d, max_tokens=70).context == 70
    eos = hf["text_config"]["eos_token_id"]
    caption = " ".join(words[i % 40] for i in range(100))
    ids, lens = opted.tokenize([caption])
    plain = tk.Tokenizer.from_file(os.path.join(d, "tokenizer.json")).encode(caption, add_special_tokens=False).ids
    assert lens.tolist() == [77] and int(ids[0, -1]) == eos and opted.n_truncated == 1
    assert ids[0].tolist() == [hf["text_config"]["bos_token_id"]] + plain[:75] + [eos]           # upstream's truncation: 75 tokens + both specials
    seventy = " ".join(words[i % 40] for i in range(70))                                         # cut at 64, whole at 77
    assert opted.tokenize([seventy])[1].tolist() == [72] and opted.n_truncated == 1
    assert default.tokenize([seventy])[1].tolist() == [64] and default.n_truncated == 1
    with pytest.raises(ValueError, match="T <= 77"):
        opted.encode_text_ids(torch.zeros(1, 78, dtype=torch.int64), torch.tensor([78]))


def test_load_model_keys_the_scorer_by_max_tokens(tmp_path, monkeypatch):
    monkeypatch.setattr(EV, "_models", {})
    R.write_model_dir(tmp_path / "m", 3, R.hf_config(max_pos=77, layers=1))
    d = str(tmp_path / "m")
    a = EV.load_model("clip", d, "cpu")
    assert a.context == 64 and EV.load_model("clip", d, "cpu") is a and EV.load_model("clip", d, "cpu", max_tokens=64) is a
    b = EV.load_model("clip", d, "cpu", max_tokens=77)
    assert b is not a and b.context == 77 and EV.load_model("clip", d, "cpu", 77) is b
    suite = EV.MetricSuite("cpu", clip_dir=d, clip_max_tokens=77)
    assert suite.fake[EV.CLIP].scorer is b
    assert EV.MetricSuite("cpu", clip_dir=d).fake[EV.CLIP].scorer.context == 64


# ------------------------------------------------------------------------------------------ the command lines
def test_flag_on_the_three_parsers(monkeypatch):
    import inspect
    import xmc_gan.clip_score as cs
    import xmc_gan.sample as sample
    import xmc_gan.train_gan as tg
    monkeypatch.delenv("XMC_CLIP_DIR", raising=False)
    assert tg.parse_args([]).clip_max_tokens == 64 and tg.parse_args(["--clip_max_tokens", "77"]).clip_max_tokens == 77
    assert cs.parse_args(["imgs", "--captions", "c.txt"]).clip_max_tokens == 64
    assert cs.parse_args(["imgs", "--captions", "c.txt", "--clip_max_tokens", "257"]).clip_max_tokens == 257
    base = ["--cfg", "x.yml", "--checkpoint", "g.pth", "--out", "o", "--synthetic", "2"]
    assert sample.parse_args(base).clip_max_tokens == 64 and sample.parse_args(base + ["--clip_max_tokens", "77"]).clip_max_tokens == 77
    for fn in (tg.eval, tg.train, EV.MetricSuite.__init__):
        assert inspect.signature(fn).parameters["clip_max_tokens"].default == 64
    assert inspect.signature(EV.load_model).parameters["max_tokens"].default == 64
    assert inspect.signature(CLIPScorer.__init__).parameters["max_tokens"].default == 64
    assert tg._clip_tokens_arg(64) == {} and tg._clip_tokens_arg(77) == {"clip_max_tokens": 77}      # off: the calls they were


# ------------------------------------------------------------------------------------------ the C ABI, without a GPU
def test_header_binding_makefile_and_op_agree_on_the_entry_point():
    name = "xmc_attention_long"
    hdr = open(os.path.join(ROOT, "include", "xmc_gan_hip.h")).read()
    assert re.search(r"#define XMC_ABI_VERSION (\d+)", hdr).group(1) == "13" and L.ABI_VERSION == 13            # an addition under 13
    before = hdr[:hdr.index("#define XMC_ABI_VERSION")]
    assert name in before and "csrc/attention_long.hip" in before
    assert name not in hdr[hdr.index("Added under 13"):hdr.index("csrc/clip.hip). */")]                        # a note of its own
    src = open(os.path.join(ROOT, "xmc-gan_amd", "csrc", "attention_long.hip")).read()
    assert re.search(rf"^int {name}\(", hdr, re.M) and f'extern "C" int {name}(' in src and name in L.EXPORTS
    assert "atomic" not in src.split("#include", 1)[1]                                                        # one writer per element, a fixed order
    assert "mfma_f32_32x32x2f32" in src and "xmc_note_kernel" in src
    assert "attention_long.hip" in re.search(r"^SRCS = (.*)$", open(os.path.join(ROOT, "xmc-gan_amd", "csrc", "Makefile")).read(), re.M).group(1)
    assert callable(ops.attention_long) and ops.attention_long.__module__.endswith("ops._forward")
    assert ops.ATTENTION_LONG_MAX_T == 1024 and ops.ATTENTION_MAX_T == 64
    for variant in ("bf16", "f16"):
        lib = L.load(variant)
        assert lib.xmc_abi_version() == 13 and hasattr(lib, name)


def test_entry_point_validates_before_any_launch():
    """NULL -> XMC_EINVAL, a shape that is not built -> XMC_ESHAPE, a misaligned pointer -> XMC_EALIGN: all return before a launch, so they
    are checked with made-up addresses that nothing dereferences"""
    lib = L.load("bf16")
    A, M = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 4)          # 16-byte aligned; 4-byte aligned only
    O = ctypes.c_void_p((1 << 20) + 2)                                       # not even 4-byte aligned
    EINVAL, EALIGN, ESHAPE = -1, -2, -3
    good = [A, A, A, 2, 77, 2, 64, 1, None]                                  # qkv, lens, out, B, T, heads, head_dim, causal, stream
    cases = ((EINVAL, [(0, None), (2, None)]),
             (ESHAPE, [(6, 32), (6, 128), (4, 0), (4, -3), (4, 1025), (3, 0), (3, -1), (5, 0), (5, -1)]),
             (EALIGN, [(0, M), (2, M), (0, O), (1, O)]))
    for rc, changes in cases:
        for i, v in changes:
            args = list(good)
            args[i] = v
            assert lib.xmc_attention_long(*args) == rc, (i, v)
    with pytest.raises(L.XmcHipError, match="XMC_ESHAPE"):
        L.check(lib.xmc_attention_long(A, None, A, 1, 1025, 1, 64, 0, None), "xmc_attention_long")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.attention_long(torch.zeros(4, 192), None, 1, 4, 1)
