"""CLIPScore on the GPU: each kernel of csrc/clip.hip alone, both towers of `CLIPScorer` whole (tiny, and one layer at ViT-B/32's geometry),
determinism, independence from what follows a caption's EOS, and the metric end to end through `MetricSuite` and `eval()` -- against
tests/clip_ref.py computed on the CPU in f64 (the resize: against Pillow, bit for bit).  Nothing outside the repository is read: weights and
model directories are generated from seeds.

Error figure of every float comparison: the largest absolute error over the reference's rms.  Bars are 1.5 x the figure measured on the
MI355X (the project's ratchet rule), written beside each constant; in this all-f32 path anything above 1e-3 would be a bug, not a bar."""
import logging
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ref as R
import xmc_gan_amd.lib as L
from xmc_gan_amd import ops
from xmc_gan_amd.clip import CLIPScorer

DEV = torch.device("cuda", 0)
WORDS = ("a man riding wave on top of surfboard two dogs play in the green grass plate food with broccoli and rice people standing near "
         "large clock tower cat sits wooden bench").split()


@pytest.fixture(autouse=True)
def _restore():
    yield
    ops.set_precision("bf16")
    from xmc_gan.config import gan
    gan.reset_cfg()


def _err(got, want):
    want = torch.as_tensor(want).double()
    return float((got.detach().double().cpu() - want).abs().max() / want.pow(2).mean().sqrt())


def _rn(*shape, seed, std=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * std


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """(directory, hf, weights) of the tiny model: width 128, 2 heads, 2 layers, 32 px in 8 px patches (17 tokens), 60 ids, 24 positions"""
    d = tmp_path_factory.mktemp("clip") / "clip-tiny"
    hf, w = R.write_model_dir(d, 5, R.hf_config(), tokenizer=R.word_tokenizer(sorted(set(WORDS))))
    return str(d), hf, w


@pytest.fixture(scope="module")
def b32(tmp_path_factory):
    """one layer per tower at ViT-B/32's geometry: vision 768 wide, 12 heads, 224 / 32 (50 tokens), FFN 3072; text 512 wide, 8 heads"""
    d = tmp_path_factory.mktemp("clip") / "clip-b32-1layer"
    hf = R.hf_config(width=768, layers=1, heads=12, ffn=3072, image=224, patch=32, vocab=1000, max_pos=77, dim=512,
                     text=dict(width=512, heads=8, ffn=2048))
    hf, w = R.write_model_dir(d, 6, hf)
    return str(d), hf, w


# ------------------------------------------------------------------------------------------ the resize: equal to Pillow
@pytest.mark.parametrize("shape", R.RESIZE_SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
def test_resize_equals_pillow(shape):
    """three images per call (the batch stride), random bytes with saturated blocks: every pixel equal to PIL.Image.resize(BICUBIC)"""
    from PIL import Image
    (h, w), (oh, ow) = shape
    img = R.sample_images(3, h, w, seed=h * 1000 + w)
    want = np.stack([np.asarray(Image.fromarray(i).resize((ow, oh), Image.BICUBIC)) for i in img])
    got = ops.resize_bicubic_u8(torch.from_numpy(img).to(DEV), oh, ow)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, oh, ow, 3)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert np.array_equal(R.pil_bicubic(img, oh, ow), want)           # (and the restatement the other tests lean on)


@pytest.mark.parametrize("h,w,short,patch", [(256, 256, 224, 32), (40, 60, 32, 8), (60, 40, 32, 8)])
def test_patch_rows_equal_the_restatement(h, w, short, patch):
    """resize + centre crop (on the long side) + table look-up + patch order, exactly: integers, one f32 table, a permutation"""
    img = R.sample_images(3, h, w, seed=h + w)
    want = R.patch_rows(R.preprocess(img, short, short), patch)
    got = ops.clip_patch_rows(torch.from_numpy(img).to(DEV), short, short, patch, torch.from_numpy(R.lut()).to(DEV))
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert torch.equal(got.cpu(), torch.from_numpy(want))


# ------------------------------------------------------------------------------------------ kernels alone
ATT_BAR = {7: 1.5 * 4.433e-07, 64: 1.5 * 1.240e-06}          # 1.5 x measured


@pytest.mark.parametrize("T", [7, 64])
def test_attention_causal(T):
    B, heads = 3, 2
    H = heads * 64
    qkv = _rn(B * T, 3 * H, seed=T)
    q, k, v = (t.reshape(B, T, H).double() for t in qkv.split(H, dim=1))
    want = R.attention(q, k, v, heads, causal=True).reshape(B * T, H)
    got = ops.attention_causal(qkv.to(DEV), B, T, heads)
    e = _err(got, want)
    print(f"attention_causal T {T}: {e:.3e}")
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got.view(B, T, H)[:, 0].cpu(), qkv.view(B, T, 3 * H)[:, 0, 2 * H:])        # query 0 sees key 0 alone: v[0]
    assert e <= ATT_BAR[T]
    with pytest.raises(AssertionError):
        ops.attention_causal(torch.zeros(65, 3 * 64, device=DEV), 1, 65, 1)
    with pytest.raises(RuntimeError):
        ops.attention_causal(qkv, B, T, heads)


QGELU_BAR = 1.5 * 2.691e-07          # 1.5 x measured


def test_bias_quick_gelu():
    """21 rows of 256 with |x + bias| up to 50: finite at both ends"""
    x, bias = _rn(21, 256, seed=1, std=3.0), _rn(256, seed=2)
    x[0, :8] = torch.tensor([50.0, -50.0, 49.0, -49.0, 30.0, -30.0, 0.0, -0.0]) - bias[:8]
    want = R.quick_gelu((x + bias).double())
    got = ops.bias_quick_gelu(x.to(DEV), bias.to(DEV))
    e = _err(got, want)
    print(f"bias_quick_gelu: {e:.3e}")
    assert bool(torch.isfinite(got).all()) and e <= QGELU_BAR
    with pytest.raises(L.XmcHipError):
        ops.bias_quick_gelu(torch.zeros(4, 12, device=DEV), torch.zeros(12, device=DEV))


EMBED_BAR = {("vision", 128): 1.5 * 2.719e-07, ("vision", 768): 1.5 * 4.513e-07, ("text", 128): 1.5 * 1.675e-07,
             ("text", 768): 1.5 * 1.668e-07, ("pool", 128): 1.5 * 3.538e-07, ("pool", 768): 1.5 * 4.029e-07}          # 1.5 x measured


@pytest.mark.parametrize("width", [128, 768])
def test_embed_and_pool_kernels(width):
    """3 images of 5 patch rows (18 rows: not a multiple of the 4 rows a workgroup takes), a mean far from zero"""
    N, GG = 3, 5
    patch, cls, pos = _rn(N * GG, width, seed=1) + 2.0, _rn(width, seed=2), _rn(GG + 1, width, seed=3)
    gamma, beta = 1 + 0.1 * _rn(width, seed=4), _rn(width, seed=5)
    rows = torch.cat([cls.expand(N, 1, width), patch.view(N, GG, width)], 1).double() + pos.double()
    want = R.layer_norm(rows, gamma.double(), beta.double(), 1e-5).reshape(N * (GG + 1), width)
    d = lambda t: t.to(DEV).contiguous()      # noqa: E731
    got = ops.clip_vision_embed(d(patch), d(cls), d(pos), d(gamma), d(beta), 1e-5)
    e = _err(got, want)
    print(f"clip_vision_embed width {width}: {e:.3e}")
    assert e <= EMBED_BAR["vision", width]

    B, T, V = 3, 7, 50
    tok, tpos = _rn(V, width, seed=6), _rn(T + 2, width, seed=7)
    ids = torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(8))
    ids[0, 0], ids[1, 1] = 0, V - 1
    want = (tok.double()[ids] + tpos.double()[:T]).reshape(B * T, width)
    got = ops.clip_text_embed(ids.to(DEV), d(tok), d(tpos))
    e = _err(got, want)
    print(f"clip_text_embed width {width}: {e:.3e}")
    assert e <= EMBED_BAR["text", width]
    bad = ids.clone()
    bad[2, 3] = V                                             # outside the table: a zero row, nothing read
    assert bool((ops.clip_text_embed(bad.to(DEV), d(tok), d(tpos)).view(B, T, width)[2, 3] == 0).all())

    x = _rn(B * T, width, seed=9) * 2 + 3
    index = torch.tensor([6, 0, 3], dtype=torch.int32)
    want = R.layer_norm(x.view(B, T, width)[torch.arange(B), index.long()].double(), gamma.double(), beta.double(), 1e-5)
    got = ops.clip_pool_ln(d(x), index.to(DEV), T, d(gamma), d(beta), 1e-5)
    e = _err(got, want)
    print(f"clip_pool_ln width {width}: {e:.3e}")
    assert tuple(got.shape) == (B, width) and e <= EMBED_BAR["pool", width]
    with pytest.raises(L.XmcHipError):                     # a width that is not built is refused, not computed wrong
        ops.clip_pool_ln(torch.zeros(B * T, 96, device=DEV), index.to(DEV), T, torch.ones(96, device=DEV), torch.zeros(96, device=DEV), 1e-5)


COS_BAR = 1.5 * 1.192e-07          # 1.5 x measured (absolute: a cosine; the largest is one f32 ulp of the cosine 1 of parallel rows)


def test_cosine_rows_and_pairing():
    img, txt = _rn(7, 64, seed=1), _rn(3, 64, seed=2)
    cap = torch.tensor([0, 0, 1, 2, 2, 1, 0], dtype=torch.int32)
    got = ops.clip_cosine(img.to(DEV), txt.to(DEV), cap.to(DEV)).cpu().double()
    e = float((got - R.cosine(img, txt[cap.long()])).abs().max())
    same = ops.clip_cosine(img[:3].to(DEV), txt.to(DEV)).cpu().double()
    e = max(e, float((same - R.cosine(img[:3], txt)).abs().max()))
    parallel = ops.clip_cosine(txt.to(DEV), (2.0 * txt).to(DEV)).cpu().double()          # a row and twice that row: 1, whatever the norms
    e = max(e, float((parallel - 1.0).abs().max()))
    print(f"clip_cosine: {e:.3e}")
    assert e <= COS_BAR
    with pytest.raises(AssertionError):
        ops.clip_cosine(img.to(DEV), txt.to(DEV))                     # seven images, three captions, no pairing


# ------------------------------------------------------------------------------------------ one copy of the device code, bit for bit
@pytest.mark.parametrize("T", [7, 64])
def test_causal_attention_is_short_attention_with_growing_lengths(T):
    """one sample T times with the lengths 1 .. T: query b of the sample that is b + 1 tokens long sees the keys 0 .. b, as causal query b does"""
    heads = 2
    H = heads * 64
    qkv = _rn(T, 3 * H, seed=40 + T).to(DEV)
    lens = torch.arange(1, T + 1, dtype=torch.int32, device=DEV)
    short = ops.attention_short(qkv.repeat(T, 1), lens, T, T, heads).view(T, T, H)
    causal = ops.attention_causal(qkv, 1, T, heads)
    assert torch.equal(short[torch.arange(T), torch.arange(T)], causal)


@pytest.mark.parametrize("width", [128, 768])
def test_embed_and_pool_layernorms_are_add_layernorm(width):
    """the LayerNorm of `clip_pool_ln` and of `clip_vision_embed` on rows that `add_layernorm` is handed ready-made"""
    N, GG, T = 3, 4, 5
    d = lambda t: t.to(DEV).contiguous()      # noqa: E731
    gamma, beta = d(1 + 0.1 * _rn(width, seed=4)), d(_rn(width, seed=5))
    x = d(_rn(N * T, width, seed=9) * 2 + 3)
    index = torch.tensor([0, T - 1, 2], dtype=torch.int32)
    want, _ = ops.add_layernorm(d(x.view(N, T, width)[torch.arange(N), index.long()]), None, gamma, beta, 1e-5)
    assert torch.equal(ops.clip_pool_ln(x, index.to(DEV), T, gamma, beta, 1e-5), want)

    patch, cls, pos = d(_rn(N * GG, width, seed=1) + 2.0), d(_rn(width, seed=2)), d(_rn(GG + 1, width, seed=3))
    rows = torch.cat([cls.expand(N, 1, width), patch.view(N, GG, width)], 1).reshape(N * (GG + 1), width).contiguous()
    want, _ = ops.add_layernorm(rows, pos.repeat(N, 1), gamma, beta, 1e-5)
    assert torch.equal(ops.clip_vision_embed(patch, cls, pos, gamma, beta, 1e-5), want)


# ------------------------------------------------------------------------------------------ the towers
TOWER_BAR = {("tiny", "image"): 1.5 * 1.080e-06, ("tiny", "text"): 1.5 * 1.242e-06, ("b32", "image"): 1.5 * 5.937e-06,
             ("b32", "text"): 1.5 * 3.548e-06}          # 1.5 x measured (tiny: the larger of the two activations)


def _towers(model, which, n_img, hw, lengths, T):
    d, hf, w = model
    sc = CLIPScorer(d, DEV)
    img = R.sample_images(n_img, hw[0], hw[1], seed=3)
    size = hf["vision_config"]["image_size"]
    want = R.image_features(w, hf, torch.from_numpy(R.preprocess(img, size, size)))
    got = sc.encode_images(torch.from_numpy(img).to(DEV))
    e = _err(got, want)
    print(f"{which} image tower: {e:.3e}")
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape) and e <= TOWER_BAR[which, "image"]
    ids, lens = R.random_ids(hf, lengths, T, seed=4)
    want = R.text_features(w, hf, ids, lens)
    got = sc.encode_text_ids(ids, lens)
    e = _err(got, want)
    print(f"{which} text tower: {e:.3e}")
    assert tuple(got.shape) == tuple(want.shape) and e <= TOWER_BAR[which, "text"]
    return sc


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
def test_both_towers_tiny(tiny, tmp_path, act):
    if act == "gelu":
        d = tmp_path / "clip-tiny-gelu"
        hf, w = R.write_model_dir(d, 5, R.hf_config(act="gelu"))
        tiny = (str(d), hf, w)
    ops.set_precision("bf16")                                  # f32 whatever the precision mode says
    _towers(tiny, "tiny", 3, (40, 60), [9, 5, 2], 9)


def test_one_layer_at_vit_b32_geometry(b32):
    _towers(b32, "b32", 2, (256, 256), [20, 11], 20)


def test_nothing_after_the_eos_reaches_a_feature_and_runs_repeat(tiny):
    d, hf, _ = tiny
    sc = CLIPScorer(d, DEV)
    lengths = [9, 5, 2, 7]
    short, lens = R.random_ids(hf, lengths, 9, seed=4)
    long_, _ = R.random_ids(hf, lengths, 24, seed=4, fill="noise")
    assert torch.equal(short[:, :2], long_[:, :2])
    a, b = sc.encode_text_ids(short, lens), sc.encode_text_ids(long_, lens)
    assert torch.equal(a, b)                                          # the same bytes at T = 9 and T = 24
    assert torch.equal(a, sc.encode_text_ids(short, lens))            # and twice
    img = torch.from_numpy(R.sample_images(3, 40, 60, seed=3)).to(DEV)
    f1, f2 = sc.encode_images(img), sc.encode_images(img)
    assert torch.equal(f1, f2)
    c = torch.tensor([0, 3, 1], dtype=torch.int32)
    assert torch.equal(sc.score(f1, a, c), sc.score(f2, b, c))


# ------------------------------------------------------------------------------------------ the metric, end to end
SCORE_BAR = {"suite": 1.5 * 1.187e-06, "eval": 1.5 * 1.796e-06}       # 1.5 x measured (absolute, on clip_score, its std and 100 x the mean cosine)


def _reference_score(model, u8_batches):
    """the restatement's (clip_score, std, cosine) for [(uint8 [N,H,W,3], captions, caption_of_image)]"""
    d, hf, w = model
    import tokenizers
    tok = tokenizers.Tokenizer.from_file(os.path.join(d, "tokenizer.json"))
    tc, size = hf["text_config"], hf["vision_config"]["image_size"]
    cos = []
    for u8, captions, pairing in u8_batches:
        rows = [[tc["bos_token_id"]] + tok.encode(c, add_special_tokens=False).ids + [tc["eos_token_id"]] for c in captions]
        T = max(map(len, rows))
        ids = torch.tensor([r + [0] * (T - len(r)) for r in rows])
        txt = R.text_features(w, hf, ids, torch.tensor([len(r) for r in rows]))
        img = R.image_features(w, hf, torch.from_numpy(R.preprocess(u8.cpu().numpy(), size, size)))
        cos.append(R.cosine(img, txt[torch.as_tensor(pairing).long()]))
    return R.clip_score(torch.cat(cos))


def test_metric_suite_end_to_end(tiny):
    from xmc_gan_amd.evaluate import CLIP, MetricSuite
    caps = ["a man riding a wave", "two dogs play in the green grass", "the cat sits on a wooden bench"]
    batches = [(torch.from_numpy(R.sample_images(6, 40, 40, seed=1)).to(DEV), caps, [0, 0, 1, 1, 2, 2]),
               (torch.from_numpy(R.sample_images(2, 40, 40, seed=2)).to(DEV), caps[:2], None)]
    suite = MetricSuite(DEV, clip_dir=tiny[0])
    for u8, c, pairing in batches:
        suite.update_fake(u8, None, None if pairing is None else torch.tensor(pairing), captions=c)
    (metric, values, why), = list(suite.results())
    want = _reference_score(tiny, [(u8, c, range(len(c)) if p is None else p) for u8, c, p in batches])
    e = max(abs(values["clip_score"] - want[0]), abs(values["std"] - want[1]), 100 * abs(values["cosine"] - want[2]))
    print(f"MetricSuite clip_score {values['clip_score']:.6f} against {want[0]:.6f}; it, std and 100 x cosine within {e:.3e}")
    assert metric == CLIP and why is None and list(values) == ["clip_score", "std", "cosine", "n", "n_truncated", "model"]
    assert values["n"] == 8 and values["n_truncated"] == 0 and values["model"] == "clip-tiny"
    assert e <= SCORE_BAR["suite"]


def test_eval_logs_the_line_and_the_scalar(tiny, tmp_path, monkeypatch):
    """`eval(clip_dir=)` on a WORD-caption loader: the caption strings come through the dataset's i2w; the line, the scalar and the
    'clip_score_*' metrics carry the restatement's score of the very images and captions the metric saw"""
    import xmc_gan.train_gan as tg
    from test_sample_gpu import _use_cfg, _yml
    from xmc_gan.model.encoder import RNN_ENCODER
    from xmc_gan_amd import clip as CL
    cfg = _use_cfg(_yml(tmp_path))
    torch.manual_seed(2)
    netG = tg.build_models(DEV)[0]
    text = RNN_ENCODER(cfg).to(DEV).eval()
    loader = tg.SyntheticCOCO(2, 4, cfg.IMG.SIZE, cfg.TEXT.MAX_LENGTH, 1, cfg.TEXT.VOCA_SIZE, distinct=2)
    words = sorted(set(WORDS))
    seen = []
    update = CL.CLIPScoreStats.update
    monkeypatch.setattr(CL.CLIPScoreStats, "update", lambda self, u8, c, p=None: (seen.append((u8.clone(), list(c), p)), update(self, u8, c, p))[1])
    lines, rows, metrics = [], [], {}
    logger = logging.getLogger("clip-eval-test")
    logger.setLevel(logging.INFO)
    handler = logging.Handler()
    handler.emit = lambda rec: lines.append(rec.getMessage())
    logger.handlers[:] = [handler]
    logger.propagate = False
    writer = type("W", (), {"add_scalar": lambda _, tag, v, step: rows.append((tag, v, step))})()
    run = lambda **kw: tg.eval(loader=loader, state_epoch=7, text_encoder=text, netG=netG, logger=logger, num_samples=8, writer=writer,      # noqa: E731
                               metrics=metrics, **kw)
    run(clip_dir=tiny[0])                                     # no i2w (a synthetic loader): the reason line
    assert not seen and any("CLIPScore not computed: no caption text reached the metric" in l for l in lines)
    assert not any(tag == "CLIPScore" for tag, _, _ in rows)
    loader.dataset = type("D", (), {"i2w": {i: words[i % len(words)] for i in range(cfg.TEXT.VOCA_SIZE)}})()
    del lines[:], rows[:]
    run(clip_dir=tiny[0])
    assert len(seen) == 2 and all(len(c) == 4 and all(isinstance(s, str) and s for s in c) for _, c, _ in seen)
    want = _reference_score(tiny, [(u8, c, range(len(c))) for u8, c, _ in seen])
    line, = [l for l in lines if "CLIPScore" in l]
    value, = [v for tag, v, step in rows if tag == "CLIPScore" and step == 7]
    e = max(abs(value - want[0]), abs(metrics["clip_score_std"] - want[1]), 100 * abs(metrics["clip_score_cosine"] - want[2]))
    print(f"eval() CLIPScore {value:.6f} against {want[0]:.6f}; it, std and 100 x cosine within {e:.3e}")
    assert e <= SCORE_BAR["eval"] and metrics["clip_score"] == value and metrics["clip_score_n"] == 8 and metrics["clip_score_model"] == "clip-tiny"
    assert line == f" epoch 7, CLIPScore : {value} +- {metrics['clip_score_std']} (n=8, model=clip-tiny)"
    del lines[:], rows[:]
    run()                                                     # without the directory: as before
    assert not any("CLIPScore" in l for l in lines) and not any(tag == "CLIPScore" for tag, _, _ in rows)


def test_sample_manifest_and_the_command_line_agree(tiny, tmp_path, capsys):
    """`sample.py --clip_score` scores what it sampled; `clip_score.py` on the PNGs it wrote, with the same batches, gives the same values"""
    import json
    import pickle
    import xmc_gan.clip_score as cli
    import xmc_gan.sample as sample
    import xmc_gan.train_gan as tg
    from test_sample_gpu import _use_cfg, _yml
    yml = _yml(tmp_path)
    _use_cfg(yml)
    torch.manual_seed(0)
    torch.save(tg.build_models(DEV)[0].state_dict(), tmp_path / "netG.pth")
    i2w = {i + 1: w for i, w in enumerate(sorted(set(WORDS)))}                 # ids 1 .. 37 of the preset's 40
    with open(tmp_path / "captions.pickle", "wb") as f:
        pickle.dump([[], [], i2w, {v: k for k, v in i2w.items()}], f)
    (tmp_path / "caps.txt").write_text("a man riding a wave\ntwo dogs play in the green grass\nthe cat sits on a wooden bench\n")
    base = ["--cfg", yml, "--checkpoint", str(tmp_path / "netG.pth"), "--data_dir", str(tmp_path), "--captions", str(tmp_path / "caps.txt"),
            "--n_per_caption", "2", "--seed", "7", "--grid_max", "0"]
    man = sample.main(base + ["--out", str(tmp_path / "a"), "--clip_score", "--clip_dir", tiny[0]])
    values = man["clip_score"]
    assert list(values) == ["clip_score", "std", "cosine", "n", "n_truncated", "model"] and (values["n"], values["model"]) == (6, "clip-tiny")
    assert values == json.load(open(tmp_path / "a" / "manifest.json"))["clip_score"] and "CLIPScore: " in capsys.readouterr().out
    assert "clip_score" not in sample.main(base + ["--out", str(tmp_path / "b")])        # not asked for: the manifest of before
    with pytest.raises(SystemExit, match="--clip_score needs a CLIP model directory"):
        sample.main(base + ["--out", str(tmp_path / "c"), "--clip_score", "--clip_dir", str(tmp_path / "nowhere")])
    # BATCH_SIZE 4 and two images per caption: the sampler's batches were files 0..3 and 4..5, and --batch 4 makes the same ones
    again = cli.main([str(tmp_path / "a"), "--captions", str(tmp_path / "caps.txt"), "--clip_dir", tiny[0], "--per_caption", "2", "--batch", "4"])
    assert again == values and json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == values
