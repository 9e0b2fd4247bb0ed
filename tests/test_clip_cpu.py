"""CPU-only checks of CLIPScore (xmc_gan_amd/clip.py, csrc/clip.hip's C ABI, the wiring in evaluate.py / train_gan.py / sample.py /
clip_score.py): tests/clip_ref.py -- what the GPU tests compare the kernels with -- against `transformers.CLIPModel`, `PIL.Image.resize`
and `transformers`' CLIP image processor; tokenisation; the loader's refusals; the entry points' declarations and argument checks; and
`MetricSuite` with a stand-in scorer."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ref as R
import xmc_gan_amd.lib as L
from xmc_gan_amd import evaluate as EV
from xmc_gan_amd import ops
from xmc_gan_amd.clip import CLIPScorer, CLIPScoreStats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("xmc_clip_resize_h_u8", "xmc_clip_resize_v_u8", "xmc_attention_causal", "xmc_bias_quick_gelu", "xmc_clip_vision_embed",
                "xmc_clip_text_embed", "xmc_clip_pool_ln", "xmc_clip_cosine")

# ------------------------------------------------------------------------------------------ the restatement against transformers
# both are f64 evaluations of the same formulas in a different operation order; error = max abs / the output's rms (outputs of order 1).
# Measured under this suite's settings (conftest.py pins the CPU code paths): quick_gelu image 3.326e-15, text 3.044e-15; gelu image
# 2.976e-15, text 4.228e-15 (with torch's default code paths: 2.714e-15, 2.368e-15, 3.064e-15, 2.537e-15).  Bar = 1.5 x the largest.
HF_BAR = 1.5 * 4.228e-15


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
def test_restatement_matches_transformers_clip_model(act):
    """The tie to the real architecture: `clip_ref.image_features` / `text_features` against a randomly initialised
    `transformers.CLIPModel` in f64 (width 128, 2 heads, 2 layers, 32 px in 8 px patches, 60 ids, 24 positions, projection 64)"""
    tr = pytest.importorskip("transformers")
    hf = R.hf_config(act=act)
    torch.manual_seed(0)
    strip = lambda c: {k: v for k, v in c.items() if k != "model_type"}      # noqa: E731
    conf = tr.CLIPConfig(text_config=strip(hf["text_config"]), vision_config=strip(hf["vision_config"]), projection_dim=hf["projection_dim"])
    model = tr.CLIPModel(conf).double().eval()
    with torch.no_grad():              # the default initialisation has unit LayerNorms and zero biases: move them
        for n, p in model.named_parameters():
            if "norm" in n or n.endswith(".bias"):
                p.add_(torch.randn_like(p) * 0.1)
            elif "proj" in n or "fc" in n:
                p.mul_(2.5)            # attention scores of order 1
    w = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert set(R.random_weights(hf, 0)) == set(w)                        # the key layout the loader reads is the one transformers writes
    px = torch.randn(3, 3, 32, 32, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    ids, lens = R.random_ids(hf, [13, 6, 2], 13, seed=1)
    with torch.no_grad():
        want_i, want_t = model.get_image_features(pixel_values=px), model.get_text_features(input_ids=ids)
    want_i, want_t = (t if torch.is_tensor(t) else t.pooler_output for t in (want_i, want_t))
    for which, got, want in (("image", R.image_features(w, hf, px), want_i), ("text", R.text_features(w, hf, ids, lens), want_t)):
        assert got.dtype == torch.float64 and got.shape == want.shape == (3, 64)
        err = float((got - want).abs().max() / want.pow(2).mean().sqrt())
        print(f"restatement vs transformers, {act} {which}: max abs error / rms = {err:.3e}")
        assert err <= HF_BAR
    # nothing after the EOS reaches a feature: the same captions in a longer, noise-filled batch
    longer, _ = R.random_ids(hf, [13, 6, 2], 20, seed=1, fill="noise")
    assert float((R.text_features(w, hf, longer, lens) - R.text_features(w, hf, ids, lens)).abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ the resize and the preprocessing
@pytest.mark.parametrize("shape", R.RESIZE_SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
def test_pil_bicubic_equals_pillow(shape):
    from PIL import Image
    (h, w), (oh, ow) = shape
    img = R.sample_images(2, h, w, seed=h * 1000 + w)
    want = np.stack([np.asarray(Image.fromarray(i).resize((ow, oh), Image.BICUBIC)) for i in img])
    assert np.array_equal(R.pil_bicubic(img, oh, ow), want)
    # the tables the kernels are handed are the restatement's: bounds, weights, zero padding up to ksize
    for n_in, n_out in ((w, ow), (h, oh)):
        bounds, coeffs, ksize = ops.pil_bicubic_tables(n_in, n_out)
        ref = R._coeffs(n_in, n_out)
        assert len(bounds) == len(coeffs) == n_out and all(len(c) == ksize for c in coeffs)
        for (xmin, cnt), c, (rmin, rk) in zip(bounds, coeffs, ref):
            assert xmin == rmin and cnt == len(rk) <= ksize and c[:cnt] == rk.tolist() and not any(c[cnt:])
            assert 0 <= xmin and xmin + cnt <= n_in and 255 * sum(map(abs, c)) + (1 << 21) < 1 << 31


PREPROCESS_BAR = 1.5 * 2.384e-07          # 1.5 x measured (max abs over the four shapes): the processor's own f32 rescale-then-normalise rounding


def test_preprocess_matches_the_transformers_image_processor():
    tr = pytest.importorskip("transformers")
    if not hasattr(tr, "CLIPImageProcessorPil"):
        pytest.skip("this transformers has no CLIPImageProcessorPil")
    from PIL import Image
    proc = tr.CLIPImageProcessorPil(size={"shortest_edge": 32}, crop_size={"height": 32, "width": 32})
    worst = 0.0
    for h, w in ((40, 60), (60, 40), (64, 64), (37, 53)):
        img = R.sample_images(2, h, w, seed=h)
        want = proc(images=[Image.fromarray(i) for i in img], return_tensors="pt")["pixel_values"]
        got = R.preprocess(img, 32, 32)
        assert got.dtype == np.float32 and got.shape == tuple(want.shape) == (2, 3, 32, 32)
        worst = max(worst, float((torch.from_numpy(got).double() - want.double()).abs().max()))
    print(f"preprocess vs CLIPImageProcessorPil: max abs = {worst:.3e}")
    assert worst <= PREPROCESS_BAR
    rows = R.patch_rows(got, 8)                                          # the GEMM operand: conv2d(stride = patch) as a product
    wgt = torch.randn(5, 3, 8, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    conv = torch.nn.functional.conv2d(torch.from_numpy(got).double(), wgt, stride=8).flatten(2).transpose(1, 2).reshape(-1, 5)
    assert float((torch.from_numpy(rows).double() @ wgt.reshape(5, -1).t() - conv).abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------ tokenisation
def _train_bpe():
    tk = pytest.importorskip("tokenizers")
    corpus = ["a man riding a wave on top of a surfboard", "two dogs play in the green grass", "a plate of food with broccoli and rice",
              "people standing near a large clock tower", "the cat sits on a wooden bench"]
    tok = tk.ByteLevelBPETokenizer(lowercase=True)
    tok.train_from_iterator(corpus, vocab_size=300, min_frequency=1, special_tokens=["<|startoftext|>", "<|endoftext|>"], show_progress=False)
    return tk, tok, corpus


def test_tokenization_adds_specials_truncates_and_pads(tmp_path, monkeypatch):
    tk, tok, corpus = _train_bpe()
    V = tok.get_vocab_size()
    hf = R.hf_config(vocab=V + 2, max_pos=12)
    R.write_model_dir(tmp_path / "m", 3, hf)
    sc = CLIPScorer(str(tmp_path / "m"))
    with pytest.raises(ImportError, match="tokenizer.json"):
        sc.tokenize(["a cat"])
    tok.save(str(tmp_path / "m" / "tokenizer.json"))
    sents = [corpus[0], "A Cat", corpus[2], "grass"]
    ids, lens = sc.tokenize(sents)
    plain = tk.Tokenizer.from_file(str(tmp_path / "m" / "tokenizer.json"))
    bos, eos = hf["text_config"]["bos_token_id"], hf["text_config"]["eos_token_id"]
    assert (sc.context, bos, eos) == (12, V, V + 1) and ids.dtype == lens.dtype == torch.int64
    want_trunc = 0
    for row, n, s in zip(ids.tolist(), lens.tolist(), sents):
        body = plain.encode(s, add_special_tokens=False).ids             # the directory's own normaliser and pre-tokeniser ("A Cat" lower-cased)
        want_trunc += len(body) > 10
        assert row[:n] == [bos] + body[:10] + [eos] and row[n:] == [0] * (len(row) - n)          # EOS stays last; padded with pad_token_id
    assert ids.shape[1] == int(lens.max()) == 12 and want_trunc >= 1 and sc.n_truncated == want_trunc
    assert plain.encode("A Cat", add_special_tokens=False).ids == plain.encode("a cat", add_special_tokens=False).ids
    # a context above the attention kernels' 64 tokens is capped there
    R.write_model_dir(tmp_path / "long", 3, R.hf_config(vocab=V + 2, max_pos=77), tokenizer=tok)
    sc = CLIPScorer(str(tmp_path / "long"))
    ids, lens = sc.tokenize([" ".join(corpus * 4)])
    assert sc.context == 64 and lens.tolist() == [64] and ids[0, -1] == eos and sc.n_truncated == 1
    monkeypatch.setitem(sys.modules, "tokenizers", None)             # without the package: the error points to encode_text_ids
    with pytest.raises(ImportError, match="encode_text_ids"):
        CLIPScorer(str(tmp_path / "long")).tokenize(["a cat"])


# ------------------------------------------------------------------------------------------ the loader
def test_loader_reads_both_weight_formats_and_the_preprocessor(tmp_path):
    hf, w = R.write_model_dir(tmp_path / "bin", 4)
    sc = CLIPScorer(str(tmp_path / "bin"))
    assert (sc.tokens, sc.grid, sc.patch, sc.dim, sc.short, sc.crop, sc.name) == (17, 4, 8, 64, 32, 32, "bin")
    assert sc.mean == R.CLIP_MEAN and sc.std == R.CLIP_STD and sc.pad_id == 0
    q = "vision_model.encoder.layers.1.self_attn."
    assert torch.equal(sc._w["v.1.wqkv"], torch.cat([w[q + n + "_proj.weight"] for n in "qkv"], 0))              # one [3W, W] weight
    assert torch.equal(sc._w["v.patch"], w["vision_model.embeddings.patch_embedding.weight"].reshape(128, 192))
    assert all(isinstance(p, torch.nn.Parameter) and not p.requires_grad and p.dtype == torch.float32 for p in sc._w.values())
    pytest.importorskip("safetensors")
    pre = dict(image_mean=[0.5, 0.4, 0.3], image_std=[0.2, 0.25, 0.3], size={"shortest_edge": 36}, crop_size={"height": 32, "width": 32}, resample=3)
    R.write_model_dir(tmp_path / "st", 4, safetensors=True, preprocessor=pre)
    st = CLIPScorer(str(tmp_path / "st"))
    assert all(torch.equal(st._w[k], sc._w[k]) for k in sc._w) and (st.short, st.crop, st.mean, st.std) == (36, 32, (0.5, 0.4, 0.3), (0.2, 0.25, 0.3))
    assert torch.equal(st.lut().cpu(), torch.from_numpy(R.lut(pre["image_mean"], pre["image_std"])))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sc.encode_images(torch.zeros(1, 32, 32, 3, dtype=torch.uint8))


def test_loader_refusals(tmp_path):
    hf = R.hf_config()
    with pytest.raises(ImportError, match="not a directory"):
        CLIPScorer(str(tmp_path / "nowhere"))
    (tmp_path / "empty").mkdir()
    with pytest.raises(ImportError, match="config.json"):
        CLIPScorer(str(tmp_path / "empty"))
    R.write_model_dir(tmp_path / "now", 1)
    os.remove(tmp_path / "now" / "pytorch_model.bin")
    with pytest.raises(ImportError, match="model.safetensors / pytorch_model.bin"):
        CLIPScorer(str(tmp_path / "now"))
    with open(tmp_path / "now" / "config.json", "w") as f:
        json.dump({k: v for k, v in hf.items() if k != "text_config"}, f)
    with pytest.raises(ImportError, match="text_config"):
        CLIPScorer(str(tmp_path / "now"))
    for i, key in enumerate(("vision_model.pre_layrnorm.weight", "vision_model.embeddings.class_embedding", "visual_projection.weight",
                             "text_model.encoder.layers.1.mlp.fc2.bias", "text_model.final_layer_norm.bias", "text_projection.weight")):
        R.write_model_dir(tmp_path / f"drop{i}", 1, drop=(key,))
        with pytest.raises(ImportError, match=re.escape(repr(key))):
            CLIPScorer(str(tmp_path / f"drop{i}"))
    R.write_model_dir(tmp_path / "shape", 1, replace={"text_model.embeddings.token_embedding.weight": torch.zeros(61, 128)})
    with pytest.raises(ValueError, match=r"token_embedding.weight is \(61, 128\)"):
        CLIPScorer(str(tmp_path / "shape"))
    for name, cfg, what in (("b16", R.hf_config(image=224, patch=16), "at most 64 tokens"), ("l14", R.hf_config(image=224, patch=14), "at most 64 tokens"),
                            ("d32", R.hf_config(width=128, heads=4), "head dimension 64"), ("wide", R.hf_config(width=1088, heads=17), "<= 1024"),
                            ("ffn", R.hf_config(ffn=260), "intermediate_size % 8"), ("act", R.hf_config(act="relu"), "hidden_act='relu'"),
                            ("textd32", R.hf_config(text=dict(width=64, heads=2)), "text_config has width 64 and 2 heads")):
        R.write_model_dir(tmp_path / name, 1, cfg)
        with pytest.raises(NotImplementedError, match=what):
            CLIPScorer(str(tmp_path / name))
    R.write_model_dir(tmp_path / "bilinear", 1, preprocessor=dict(resample=2))
    with pytest.raises(NotImplementedError, match="resample=2"):
        CLIPScorer(str(tmp_path / "bilinear"))
    R.write_model_dir(tmp_path / "ok", 1)
    sc = CLIPScorer(str(tmp_path / "ok"))
    ids, lens = R.random_ids(hf, [5, 3], 5, seed=0)
    with pytest.raises(ValueError, match="T <= 24"):
        sc.encode_text_ids(torch.zeros(2, 25, dtype=torch.int64), lens)
    with pytest.raises(ValueError, match="lengths"):
        sc.encode_text_ids(ids, torch.tensor([6, 3]))
    with pytest.raises(IndexError, match="vocab_size"):
        sc.encode_text_ids(ids + 60, lens)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sc.encode_text_ids(ids, lens)


# ------------------------------------------------------------------------------------------ the C ABI, without a GPU
def test_header_binding_makefile_and_ops_agree_on_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "xmc_gan_hip.h")).read()
    assert re.search(r"#define XMC_ABI_VERSION (\d+)", hdr).group(1) == "13" and L.ABI_VERSION == 13            # additions only
    note = hdr[hdr.index("Added under 13"):hdr.index("#define XMC_ABI_VERSION")]
    assert all(n in note for n in ENTRY_POINTS) and "csrc/clip.hip" in note
    src = open(os.path.join(ROOT, "xmc-gan_amd", "csrc", "clip.hip")).read()
    for n in ENTRY_POINTS:
        assert re.search(rf"^int {n}\(", hdr, re.M) and f'extern "C" int {n}(' in src and n in L.EXPORTS, n
    assert "clip.hip" in re.search(r"^SRCS = (.*)$", open(os.path.join(ROOT, "xmc-gan_amd", "csrc", "Makefile")).read(), re.M).group(1)
    assert "atomic" not in src.split("#include")[1]                      # one writer per element, a fixed order
    for name in ("resize_bicubic_u8", "clip_patch_rows", "attention_causal", "bias_quick_gelu", "clip_vision_embed", "clip_text_embed",
                 "clip_pool_ln", "clip_cosine"):
        assert callable(getattr(ops, name)) and getattr(ops, name).__module__.endswith("ops._forward")
    for variant in ("bf16", "f16"):
        lib = L.load(variant)
        assert lib.xmc_abi_version() == 13 and all(hasattr(lib, n) for n in ENTRY_POINTS)


def test_entry_points_validate_before_any_launch():
    """NULL -> XMC_EINVAL, a shape that is not built -> XMC_ESHAPE, a misaligned pointer -> XMC_EALIGN: all three return before a launch, so
    they are checked here with made-up addresses that nothing dereferences"""
    lib = L.load("bf16")
    A, M = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 4)          # 16-byte aligned; 4-byte aligned only
    O = ctypes.c_void_p((1 << 20) + 2)                                       # not even 4-byte aligned
    EINVAL, EALIGN, ESHAPE = -1, -2, -3
    none = lambda *idx: [(i, None) for i in idx]      # noqa: E731
    at = lambda p, *idx: [(i, p) for i in idx]        # noqa: E731
    eps = ctypes.c_float(1e-5)
    cases = {       # name: (arguments that pass every check, [(index, value)] that make them invalid / a shape that is not built / misaligned)
        "xmc_clip_resize_h_u8": ([A, A, A, A, 1, 8, 8, 4, 7, None], none(0, 1, 2, 3), [(4, 0), (7, 0), (8, 0), (8, 5000)], at(O, 2, 3)),
        "xmc_clip_resize_v_u8": ([A, A, A, A, A, 1, 8, 8, 4, 7, 1, 4, 2, 0, 2, None], none(0, 1, 2, 3, 4) + [(10, 2)],
                                 [(5, 0), (8, 0), (11, 5), (12, 3), (13, 1), (14, 5)], at(O, 1, 2, 3, 4)),
        "xmc_attention_causal": ([A, A, 2, 7, 2, 64, None], none(0, 1), [(2, 0), (3, 65), (3, 0), (4, 0), (5, 32)], [(0, M), (1, O)]),
        "xmc_bias_quick_gelu": ([A, A, A, 4, 16, None], none(0, 1, 2), [(3, 0), (4, 0)], at(M, 0, 1, 2) + [(4, 12)]),
        "xmc_clip_vision_embed": ([A, A, A, A, A, A, 2, 4, 128, eps, None], none(0, 1, 2, 3, 4, 5), [(6, 0), (7, 0), (8, 96), (8, 1088)],
                                  at(M, 0, 1, 2, 3, 4, 5)),
        "xmc_clip_text_embed": ([A, A, A, A, 2, 7, 128, 60, 24, None], none(0, 1, 2, 3), [(4, 0), (5, 25), (6, 100), (7, 0), (8, 0)],
                                at(M, 0, 1, 2, 3)),
        "xmc_clip_pool_ln": ([A, A, A, A, A, 2, 7, 128, eps, None], none(0, 1, 2, 3, 4), [(5, 0), (6, 0), (7, 32)], at(M, 0, 2, 3, 4) + [(1, O)]),
        "xmc_clip_cosine": ([A, A, A, A, 3, 3, 64, None], none(0, 1, 3), [(4, 0), (5, 0), (6, 0)], at(O, 0, 1, 2, 3)),
    }
    assert set(cases) == set(ENTRY_POINTS)
    for name, (good, invalid, shape, align) in cases.items():
        fn = getattr(lib, name)
        for rc, changes in ((EINVAL, invalid), (ESHAPE, shape), (EALIGN, align)):
            for i, v in changes:
                args = list(good)
                args[i] = v
                assert fn(*args) == rc, (name, i, v)
    assert lib.xmc_clip_cosine(A, A, None, A, 4, 3, 64, None) == ESHAPE       # the identity pairing needs a caption row per image
    with pytest.raises(L.XmcHipError, match="XMC_ESHAPE"):
        L.check(lib.xmc_attention_causal(A, A, 1, 65, 1, 64, None), "xmc_attention_causal")


# ------------------------------------------------------------------------------------------ MetricSuite with a stand-in scorer
class _Scorer:
    """stands in for CLIPScorer on the host: features are functions of the pixels / the characters, the cosine is exact"""
    name, n_truncated = "stub-clip", 0

    def __init__(self):
        self.texts, self.images = [], 0

    def encode_text(self, sentences):
        self.texts.append(list(sentences))
        self.n_truncated += sum(len(s) > 20 for s in sentences)
        return torch.stack([torch.tensor([len(s), s.count("a") - 2.0, 1.0]) for s in sentences])

    def encode_images(self, u8):
        self.images += u8.shape[0]
        f = u8.float().mean((1, 2))
        return f - f.mean(1, keepdim=True) + torch.tensor([0.0, 0.0, 1.0])

    def score(self, img, txt, caption_of_image=None):
        return R.cosine(img, txt[caption_of_image.long()]).float()


def _images(n, seed):
    return torch.randint(0, 256, (n, 4, 4, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def test_metric_suite_with_a_stub_scorer(monkeypatch):
    stub, asked = _Scorer(), []
    monkeypatch.setattr(EV, "_models", {})
    monkeypatch.setattr(EV, "load_model", lambda kind, path, device: (asked.append((kind, path)), stub)[1])
    # off: what it was
    plain = EV.MetricSuite("cpu")
    plain.update_fake(_images(3, 1), None, None, captions=["x", "y", "z"])
    assert plain.fake == {} and plain.why == {} and list(plain.results()) == [] and asked == []
    # on, and no caption text: the reason
    suite = EV.MetricSuite("cpu", clip_dir="/models/stub-clip")
    assert asked == [("clip", "/models/stub-clip")] and list(suite.fake) == [EV.CLIP] and not suite.wants_real
    suite.update_fake(_images(3, 1))
    assert list(suite.results()) == [(EV.CLIP, None, "no caption text reached the metric")] and stub.images == 0
    # one caption per image; then fewer captions and caption_of_image: each distinct caption of a batch is encoded once
    caps = ["a banana on a table", "a cat", "a banana on a table", "a very long caption about nothing at all"]
    suite.update_fake(_images(4, 2), None, None, captions=caps)
    suite.update_fake(_images(6, 3), None, torch.tensor([0, 0, 1, 1, 2, 2]), captions=[caps[1], caps[1], caps[3]])
    assert stub.texts == [[caps[0], caps[1], caps[3]], [caps[1], caps[3]]] and stub.images == 10
    (metric, values, why), = list(suite.results())
    per_image = caps + [caps[1]] * 4 + [caps[3]] * 2
    img = torch.cat([stub.encode_images(_images(4, 2)), stub.encode_images(_images(6, 3))])
    txt = torch.stack([torch.tensor([len(s), s.count("a") - 2.0, 1.0]) for s in per_image])
    cos = R.cosine(img, txt).float().double()
    want = R.clip_score(cos)
    assert metric == EV.CLIP and why is None and list(values) == ["clip_score", "std", "cosine", "n", "n_truncated", "model"]
    assert (values["clip_score"], values["std"], values["cosine"]) == want and bool((cos < 0).any()) and want[0] > 100 * want[2]      # the clamp acts
    assert (values["n"], values["n_truncated"], values["model"]) == (10, 2, "stub-clip")
    with pytest.raises(IndexError, match="do not pair up"):
        suite.update_fake(_images(2, 4), None, None, captions=caps[:3])
    # the existing metrics keep their order in front of it
    res = list(EV.MetricSuite("cpu", "", prdc_k=2, kid=True, inception_score=10, clip_dir="/models/stub-clip").results())
    assert [m for m, _, _ in res] == [EV.PRDC, EV.KID, EV.IS, EV.CLIP]


def test_clip_score_stats_on_one_image():
    stats = CLIPScoreStats(_Scorer())
    stats.update(_images(1, 1), ["a cat"])
    v = stats.finalize()
    assert v["n"] == 1 and v["std"] == 0.0 and v["clip_score"] == max(100.0 * v["cosine"], 0.0)


# ------------------------------------------------------------------------------------------ the wiring, before a device is touched
def test_trainer_flags_and_report(monkeypatch):
    import xmc_gan.train_gan as tg
    monkeypatch.delenv("XMC_CLIP_DIR", raising=False)
    assert tg.parse_args([]).clip_dir == "" and tg.parse_args(["--clip_dir", "/m"]).clip_dir == "/m"
    assert tg.EvalOptions() == ("", 0, "", False, 100, 1000, 0) and tg._new_metric_args(tg.EvalOptions(), None, None, None, None) == {}
    line, tags, without = tg._EVAL_REPORT["CLIPScore"]
    assert line.format(epoch=7, clip_score=31.5, std=2.0, cosine=0.3, n=8, n_truncated=0, model="clip-vit-base-patch32") == \
        " epoch 7, CLIPScore : 31.5 +- 2.0 (n=8, model=clip-vit-base-patch32)"
    assert tags == ("clip_score",) and tg._EVAL_SCALAR["clip_score"] == "CLIPScore"
    assert without.format(epoch=7, cnt=8, why="x") == " epoch 7, CLIPScore not computed: x"
    assert {tg._EVAL_METRICS_KEY.get(("CLIPScore", k), k) for k in ("clip_score", "std", "cosine", "n", "n_truncated", "model")} == \
        {"clip_score", "clip_score_std", "clip_score_cosine", "clip_score_n", "clip_score_n_truncated", "clip_score_model"}
    # caption strings: SENT captions as they are, WORD captions through i2w, nothing without either
    loader = type("Loader", (), {"dataset": type("D", (), {"i2w": {1: "a", 2: "cat", 3: "sits"}})()})()
    caps, lens = torch.tensor([[1, 2, 3, 0], [2, 0, 0, 0]]), torch.tensor([3, 1])
    assert tg._caption_strings(caps, lens, loader) == ["a cat sits", "cat"]
    assert tg._caption_strings(("a cat", "a dog"), lens, object()) == ["a cat", "a dog"]
    assert tg._caption_strings(caps, lens, object()) is None
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("a device was asked for"))
    with pytest.raises(SystemExit, match="--clip_dir"):
        tg._checked_args(["--cfg", os.path.join(ROOT, "xmc_gan", "cfg", "df_gan_damsm.yml"), "--clip_dir", "/nowhere/clip"])


def test_clip_score_command_line_refuses_before_a_device_is_touched(tmp_path, monkeypatch):
    import xmc_gan.clip_score as cli
    from PIL import Image
    monkeypatch.delenv("XMC_CLIP_DIR", raising=False)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("a device was asked for"))
    imgs, model, caps = tmp_path / "imgs", tmp_path / "clip", str(tmp_path / "caps.txt")
    imgs.mkdir()
    for i in range(4):
        Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(str(imgs / f"{i}.png"))
    R.write_model_dir(model, 1)
    with open(caps, "w") as f:
        f.write("a cat\n\na dog\n")
    ok = [str(imgs), "--captions", caps, "--clip_dir", str(model), "--per_caption", "2"]
    assert len(cli._check_args(cli.parse_args(ok))[0]) == 4
    for argv, what in (([str(tmp_path / "nowhere")] + ok[1:], "is not a directory"), ([str(model)] + ok[1:], "holds no image"),
                       (ok[:3], "a CLIP model directory is needed"), (ok[:4] + [str(imgs)], "a CLIP model directory is needed"),
                       (ok[:2] + [str(tmp_path / "no.txt")] + ok[3:], "is not a file"), (ok[:5], "2 captions x --per_caption 1 = 2 were expected"),
                       (ok + ["--batch", "0"], "--batch")):
        with pytest.raises(SystemExit, match=what):
            cli.main(argv)
