"""Plain restatement of what `xmc_gan_amd.clip.CLIPScorer` computes, for the tests (a helper, not a test): both CLIP towers on the CPU in
f64 from a dict of weights in the Hugging Face `CLIPModel` key layout (pre-LayerNorm layers, QuickGELU or erf GELU, causal text
attention, the EOS row pooled); Pillow's antialiased bicubic resize of an 8-bit image in integer arithmetic (`pil_bicubic`); CLIP's
preprocessing on top of it (`preprocess`, `patch_rows`); and a writer of small random model directories from a seed.
tests/test_clip_cpu.py ties the towers to `transformers.CLIPModel`, `pil_bicubic` to `PIL.Image.resize` and `preprocess` to
`transformers`' image processor."""
import json
import math
import os

import numpy as np
import torch

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
# (input height, width) -> (output height, width): the shapes the resize is checked on
RESIZE_SHAPES = (((256, 256), (224, 224)), ((64, 64), (224, 224)), ((128, 128), (224, 224)), ((200, 300), (224, 336)),
                 ((37, 53), (32, 45)), ((224, 224), (224, 224)), ((40, 40), (32, 32)), ((16, 16), (32, 32)))


def hf_config(width=128, layers=2, heads=2, ffn=256, image=32, patch=8, vocab=60, max_pos=24, dim=64, act="quick_gelu", text=None,
              **over):
    """a CLIPModel config.json; `text`: overrides of the text tower's sizes (width, heads, ffn, layers)"""
    t = dict(width=width, layers=layers, heads=heads, ffn=ffn)
    t.update(text or {})
    cfg = dict(model_type="clip", architectures=["CLIPModel"], projection_dim=dim, logit_scale_init_value=2.6592,
               vision_config=dict(model_type="clip_vision_model", hidden_size=width, num_hidden_layers=layers, num_attention_heads=heads,
                                  intermediate_size=ffn, image_size=image, patch_size=patch, num_channels=3, hidden_act=act,
                                  layer_norm_eps=1e-5, projection_dim=dim, attention_dropout=0.0),
               text_config=dict(model_type="clip_text_model", hidden_size=t["width"], num_hidden_layers=t["layers"],
                                num_attention_heads=t["heads"], intermediate_size=t["ffn"], vocab_size=vocab,
                                max_position_embeddings=max_pos, hidden_act=act, layer_norm_eps=1e-5, projection_dim=dim,
                                attention_dropout=0.0, bos_token_id=vocab - 2, eos_token_id=vocab - 1, pad_token_id=0))
    cfg.update(over)
    return cfg


def random_weights(hf, seed):
    """f32 weights of a CLIPModel with `hf`'s sizes, Hugging Face keys: N(0, 0.05) matrices (scores of order 1 at head dimension 64),
    N(0, 0.5) embeddings, LayerNorm scales around 1, biases N(0, 0.1)"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *shape, std=1.0: torch.randn(*shape, generator=g) * std      # noqa: E731
    vc, tc, D = hf["vision_config"], hf["text_config"], hf["projection_dim"]
    w = {}

    def lin(key, out, inp):
        w[key + ".weight"], w[key + ".bias"] = rn(out, inp, std=0.05), rn(out, std=0.1)

    def ln(key, H):
        w[key + ".weight"], w[key + ".bias"] = 1.0 + rn(H, std=0.1), rn(H, std=0.1)

    def layers(root, c):
        H, F = c["hidden_size"], c["intermediate_size"]
        for i in range(c["num_hidden_layers"]):
            l = f"{root}encoder.layers.{i}."
            for n in "qkv":
                lin(l + f"self_attn.{n}_proj", H, H)
            lin(l + "self_attn.out_proj", H, H)
            ln(l + "layer_norm1", H)
            lin(l + "mlp.fc1", F, H)
            lin(l + "mlp.fc2", H, F)
            ln(l + "layer_norm2", H)

    W, P = vc["hidden_size"], vc["patch_size"]
    G = vc["image_size"] // P
    w["vision_model.embeddings.class_embedding"] = rn(W, std=0.5)
    w["vision_model.embeddings.patch_embedding.weight"] = rn(W, 3, P, P, std=0.05)
    w["vision_model.embeddings.position_embedding.weight"] = rn(G * G + 1, W, std=0.5)
    ln("vision_model.pre_layrnorm", W)
    layers("vision_model.", vc)
    ln("vision_model.post_layernorm", W)
    w["visual_projection.weight"] = rn(D, W, std=0.05)
    TW = tc["hidden_size"]
    w["text_model.embeddings.token_embedding.weight"] = rn(tc["vocab_size"], TW, std=0.5)
    w["text_model.embeddings.position_embedding.weight"] = rn(tc["max_position_embeddings"], TW, std=0.5)
    layers("text_model.", tc)
    ln("text_model.final_layer_norm", TW)
    w["text_projection.weight"] = rn(D, TW, std=0.05)
    w["logit_scale"] = torch.tensor(2.6592)           # a key the loader must ignore
    return w


def write_model_dir(path, seed, hf=None, safetensors=False, preprocessor=None, tokenizer=None, drop=(), replace=None):
    """a random model directory: config.json + pytorch_model.bin (or model.safetensors) [+ preprocessor_config.json] [+ tokenizer.json from
    a `tokenizers.Tokenizer`].  `drop`: weight keys left out; `replace`: {key: tensor}.  Returns (hf, weights)."""
    hf = hf or hf_config()
    w = random_weights(hf, seed)
    saved = {k: v for k, v in w.items() if k not in drop}
    saved.update(replace or {})
    d = str(path)
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(hf, f)
    if safetensors:
        from safetensors.torch import save_file
        save_file({k: v.contiguous() for k, v in saved.items()}, os.path.join(d, "model.safetensors"))
    else:
        torch.save(saved, os.path.join(d, "pytorch_model.bin"))
    if preprocessor is not None:
        with open(os.path.join(d, "preprocessor_config.json"), "w") as f:
            json.dump(preprocessor, f)
    if tokenizer is not None:
        tokenizer.save(os.path.join(d, "tokenizer.json"))
    return hf, w


def word_tokenizer(words):
    """a `tokenizers.Tokenizer` that splits on whitespace and maps each of `words` to its index + 1 (0: unknown / padding): enough of a
    tokenizer.json for the end-to-end tests"""
    import tokenizers
    vocab = {"<unk>": 0}
    vocab.update({wd: i + 1 for i, wd in enumerate(words)})
    tok = tokenizers.Tokenizer(tokenizers.models.WordLevel(vocab, unk_token="<unk>"))
    tok.pre_tokenizer = tokenizers.pre_tokenizers.Whitespace()
    return tok


# ------------------------------------------------------------------------------------------ the towers, f64
def layer_norm(x, g, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def attention(q, k, v, heads, causal):
    """q, k, v [B, T, H] -> softmax(q k^T / sqrt(d) [over keys j <= i]) v per head, [B, T, H]"""
    B, T, H = q.shape
    d = H // heads
    split = lambda t: t.view(B, T, heads, d).transpose(1, 2)      # noqa: E731
    s = split(q) @ split(k).transpose(-1, -2) / math.sqrt(d)
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(T, T, dtype=torch.bool), 1), float("-inf"))
    return (torch.softmax(s, -1) @ split(v)).transpose(1, 2).reshape(B, T, H)


def _f64(w):
    return {k: v.to(torch.float64) for k, v in w.items() if v.is_floating_point()}


def encoder_layers(W, root, c, x, causal, first=None):
    """the pre-LayerNorm layers of one tower on x [B, T, H] (the first `first` of them)"""
    act = quick_gelu if c["hidden_act"] == "quick_gelu" else gelu_erf
    lin = lambda t, key: t @ W[key + ".weight"].t() + W[key + ".bias"]      # noqa: E731
    eps, heads = c["layer_norm_eps"], c["num_attention_heads"]
    for i in range(c["num_hidden_layers"] if first is None else first):
        l = f"{root}encoder.layers.{i}."
        h = layer_norm(x, W[l + "layer_norm1.weight"], W[l + "layer_norm1.bias"], eps)
        a = l + "self_attn."
        ctx = attention(lin(h, a + "q_proj"), lin(h, a + "k_proj"), lin(h, a + "v_proj"), heads, causal)
        x = x + lin(ctx, a + "out_proj")
        h = layer_norm(x, W[l + "layer_norm2.weight"], W[l + "layer_norm2.bias"], eps)
        x = x + lin(act(lin(h, l + "mlp.fc1")), l + "mlp.fc2")
    return x


def vision_embed(W, c, pixel_values):
    """CLIPVisionEmbeddings + pre_layrnorm: pixel_values [N, 3, S, S] -> [N, G G + 1, H]"""
    P = c["patch_size"]
    x = torch.nn.functional.conv2d(pixel_values.to(torch.float64), W["vision_model.embeddings.patch_embedding.weight"], stride=P)
    x = x.flatten(2).transpose(1, 2)
    cls = W["vision_model.embeddings.class_embedding"].expand(x.shape[0], 1, -1)
    x = torch.cat([cls, x], 1) + W["vision_model.embeddings.position_embedding.weight"]
    return layer_norm(x, W["vision_model.pre_layrnorm.weight"], W["vision_model.pre_layrnorm.bias"], c["layer_norm_eps"])


def image_features(w, hf, pixel_values):
    """CLIPModel.get_image_features: [N, 3, S, S] normalised pixels -> [N, D], f64"""
    W, c = _f64(w), hf["vision_config"]
    x = encoder_layers(W, "vision_model.", c, vision_embed(W, c, pixel_values), causal=False)
    pooled = layer_norm(x[:, 0], W["vision_model.post_layernorm.weight"], W["vision_model.post_layernorm.bias"], c["layer_norm_eps"])
    return pooled @ W["visual_projection.weight"].t()


def text_embed(W, ids):
    T = ids.shape[1]
    return W["text_model.embeddings.token_embedding.weight"][ids] + W["text_model.embeddings.position_embedding.weight"][:T]


def text_features(w, hf, ids, lens):
    """CLIPModel.get_text_features with the pooled row at lens - 1 (the EOS): ids int64 [B, T] -> [B, D], f64"""
    W, c = _f64(w), hf["text_config"]
    ids, lens = torch.as_tensor(ids), torch.as_tensor(lens)
    x = encoder_layers(W, "text_model.", c, text_embed(W, ids), causal=True)
    x = layer_norm(x, W["text_model.final_layer_norm.weight"], W["text_model.final_layer_norm.bias"], c["layer_norm_eps"])
    return x[torch.arange(ids.shape[0]), lens - 1] @ W["text_projection.weight"].t()


def cosine(a, b):
    a, b = a.to(torch.float64), b.to(torch.float64)
    return (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))


def clip_score(cos):
    """(the mean of max(100 cos, 0), its standard deviation, the mean cosine) in f64: the torchmetrics convention"""
    cos = torch.as_tensor(cos, dtype=torch.float64)
    per = (100.0 * cos).clamp_min(0.0)
    return float(per.mean()), float(per.std(unbiased=False)), float(cos.mean())


def random_ids(hf, lengths, T, seed, fill="pad"):
    """int64 [B, T]: BOS tokens EOS, then the pad id (or, `fill` = 'noise', random ordinary tokens: nothing after the EOS may matter)"""
    tc = hf["text_config"]
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((len(lengths), T), tc["pad_token_id"], dtype=torch.int64)
    for b, n in enumerate(lengths):
        ids[b, 0], ids[b, n - 1] = tc["bos_token_id"], tc["eos_token_id"]
        ids[b, 1:n - 1] = torch.randint(1, tc["vocab_size"] - 2, (n - 2,), generator=g)
    if fill == "noise":
        noise = torch.randint(1, tc["vocab_size"] - 2, ids.shape, generator=torch.Generator().manual_seed(seed + 1))
        after = torch.arange(T)[None, :] >= torch.tensor(lengths)[:, None]
        ids = torch.where(after, noise, ids)
    return ids, torch.tensor(lengths, dtype=torch.int64)


# ------------------------------------------------------------------------------------------ Pillow's resize, integers
def _cubic(x):
    x = abs(x)
    if x < 1.0:
        return ((-0.5 + 2.0) * x - (-0.5 + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * -0.5
    return 0.0


def _coeffs(n_in, n_out):
    """Resample.c precompute_coeffs + normalize_coeffs_8bpc for the bicubic filter: per output sample (first input sample, int weights)"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support, ss = 2.0 * fs, 1.0 / fs
    out = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [_cubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        w = [v / ww for v in w] if ww != 0.0 else w
        out.append((xmin, np.array([int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22)) for v in w], dtype=np.int64)))
    return out


def _pass(img, n_out, axis):
    img = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((n_out,) + img.shape[1:], dtype=np.uint8)
    for xx, (xmin, k) in enumerate(_coeffs(img.shape[0], n_out)):
        acc = (1 << 21) + np.tensordot(k, img[xmin:xmin + len(k)], axes=(0, 0))
        out[xx] = np.clip(acc >> 22, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def pil_bicubic(u8, oh, ow):
    """`PIL.Image.resize((ow, oh), BICUBIC)` of a uint8 [..., H, W, 3] array in integer arithmetic: the horizontal pass into uint8, then
    the vertical one on that"""
    u8 = np.asarray(u8)
    assert u8.dtype == np.uint8 and u8.shape[-1] == 3
    return _pass(_pass(u8, ow, u8.ndim - 2), oh, u8.ndim - 3)


def resize_target(h, w, short):
    return (short, int(short * w / h)) if h <= w else (int(short * h / w), short)


def lut(mean=CLIP_MEAN, std=CLIP_STD):
    """f32 [3, 256]: (v / 255 - mean_c) / std_c in f64, rounded once"""
    v = np.arange(256, dtype=np.float64)[None, :] / 255.0
    return ((v - np.array(mean, dtype=np.float64)[:, None]) / np.array(std, dtype=np.float64)[:, None]).astype(np.float32)


def preprocess(u8, short, crop, mean=CLIP_MEAN, std=CLIP_STD):
    """CLIP's preprocessing of uint8 [N, H, W, 3]: resize the short side to `short`, centre crop, normalise -> f32 [N, 3, crop, crop]"""
    u8 = np.asarray(u8)
    oh, ow = resize_target(u8.shape[1], u8.shape[2], short)
    r = pil_bicubic(u8, oh, ow)
    top, left = (oh - crop) // 2, (ow - crop) // 2
    r = r[:, top:top + crop, left:left + crop]
    table = lut(mean, std)
    return np.stack([table[c][r[..., c]] for c in range(3)], 1)


def patch_rows(pixels, patch):
    """f32 [N, 3, S, S] -> [N (S/P)^2, 3 P P], column c P P + py P + px: the patch embedding's GEMM operand"""
    N, _, S, _ = pixels.shape
    G = S // patch
    return pixels.reshape(N, 3, G, patch, G, patch).transpose(0, 2, 4, 1, 3, 5).reshape(N * G * G, 3 * patch * patch)


def sample_images(n, h, w, seed):
    """random bytes with saturated 0 / 255 blocks (the clamps of both passes see overshoot), uint8 [n, h, w, 3]"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    img[:, : h // 3, : w // 2] = 255
    img[:, h // 2:, w // 3: 2 * w // 3] = 0
    img[:, h // 3: h // 2, w // 2:] = np.where(np.indices((h // 2 - h // 3, w - w // 2)).sum(0) % 2 == 0, 0, 255)[None, :, :, None]
    return img
