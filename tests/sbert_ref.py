"""Plain-torch restatement of what SBERT_ENCODER computes, for the tests (a helper, not a test): the RoBERTa forward -- embeddings
with RoBERTa's position ids, post-LayerNorm transformer layers, exact (erf) GELU -- and the pooling tail of the reference's
SBERT_ENCODER.forward (model/encoder.py:50-70), on the CPU in f64, from a dict of weights in the Hugging Face key layout; and a
writer of small random model directories (config.json + pytorch_model.bin) from a seed.  tests/test_sbert_cpu.py ties `hidden_states`
to `transformers.RobertaModel`."""
import json
import math
import os

import torch


def hf_config(hidden=128, layers=2, heads=2, ffn=256, vocab=60, max_pos=40, **over):
    cfg = dict(model_type="roberta", architectures=["RobertaModel"], hidden_size=hidden, num_hidden_layers=layers,
               num_attention_heads=heads, intermediate_size=ffn, vocab_size=vocab, max_position_embeddings=max_pos,
               type_vocab_size=1, hidden_act="gelu", layer_norm_eps=1e-5, pad_token_id=1, bos_token_id=0, eos_token_id=2,
               position_embedding_type="absolute", hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    cfg.update(over)
    return cfg


def random_weights(hf, seed, prefix="", pooler=False):
    """f32 weights of a RobertaModel with `hf`'s sizes, Hugging Face keys: N(0, 0.05) matrices (scores of order 1 at head dimension 64),
    N(0, 0.5) embeddings, LayerNorm scales around 1, biases N(0, 0.1)"""
    g = torch.Generator().manual_seed(seed)
    H, F = hf["hidden_size"], hf["intermediate_size"]
    rn = lambda *shape, std=1.0: torch.randn(*shape, generator=g) * std
    w = {}

    def lin(key, out, inp):
        w[key + ".weight"], w[key + ".bias"] = rn(out, inp, std=0.05), rn(out, std=0.1)

    def ln(key):
        w[key + ".weight"], w[key + ".bias"] = 1.0 + rn(H, std=0.1), rn(H, std=0.1)

    w["embeddings.word_embeddings.weight"] = rn(hf["vocab_size"], H, std=0.5)
    w["embeddings.position_embeddings.weight"] = rn(hf["max_position_embeddings"], H, std=0.5)
    w["embeddings.token_type_embeddings.weight"] = rn(hf["type_vocab_size"], H, std=0.5)
    ln("embeddings.LayerNorm")
    for i in range(hf["num_hidden_layers"]):
        l = f"encoder.layer.{i}."
        for n in ("query", "key", "value"):
            lin(l + "attention.self." + n, H, H)
        lin(l + "attention.output.dense", H, H)
        ln(l + "attention.output.LayerNorm")
        lin(l + "intermediate.dense", F, H)
        lin(l + "output.dense", H, F)
        ln(l + "output.LayerNorm")
    if pooler:            # keys a loader must ignore
        lin("pooler.dense", H, H)
        w["embeddings.position_ids"] = torch.arange(hf["max_position_embeddings"])[None]
    out = {prefix + k: v for k, v in w.items()}
    if pooler:
        out["lm_head.bias"] = rn(hf["vocab_size"])
    return out


def write_model_dir(path, seed, hf=None, subdir="", prefix="", pooler=False, safetensors=False):
    """a random model directory: config.json + pytorch_model.bin (or model.safetensors) under path/subdir.  Returns (hf, weights) with
    the weights under their un-prefixed keys."""
    hf = hf or hf_config()
    w = random_weights(hf, seed, prefix, pooler)
    d = os.path.join(str(path), subdir)
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(hf, f)
    if safetensors:
        from safetensors.torch import save_file
        save_file({k: v.contiguous() for k, v in w.items()}, os.path.join(d, "model.safetensors"))
    else:
        torch.save(w, os.path.join(d, "pytorch_model.bin"))
    return hf, {k[len(prefix):] if prefix and k.startswith(prefix) else k: v for k, v in w.items()}


def _rounder(fmt):
    return (lambda t: t) if fmt is None else (lambda t: t.to(torch.float32).to(fmt).to(torch.float64))


def layer_norm(x, g, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def attention(q, k, v, lengths, heads):
    """q, k, v [B, T, H] -> softmax(q k^T / sqrt(d) + key padding mask) v per head, [B, T, H]"""
    B, T, H = q.shape
    d = H // heads
    split = lambda t: t.view(B, T, heads, d).transpose(1, 2)
    s = split(q) @ split(k).transpose(-1, -2) / math.sqrt(d)
    key_ok = torch.arange(T)[None, :] < torch.as_tensor(lengths)[:, None]
    s = s.masked_fill(~key_ok[:, None, None, :], float("-inf"))
    return (torch.softmax(s, -1) @ split(v)).transpose(1, 2).reshape(B, T, H)


def hidden_states(w, hf, input_ids, lengths, gemm_fmt=None):
    """last hidden state [B, T, H] in f64.  `gemm_fmt` (torch.bfloat16 / torch.float16): both operands of the four GEMMs per layer
    rounded to that format first, everything else exact -- the error of the format, as an engine that feeds its matrix units 16-bit
    operands and keeps the residual stream, LayerNorm and softmax in f32 has it."""
    rnd = _rounder(gemm_fmt)
    W = {k: v.to(torch.float64) for k, v in w.items() if v.is_floating_point()}
    lin = lambda x, key: rnd(x) @ rnd(W[key + ".weight"]).t() + W[key + ".bias"]
    ids, lengths = torch.as_tensor(input_ids), torch.as_tensor(lengths)
    B, T = ids.shape
    eps, pad, heads = hf["layer_norm_eps"], hf["pad_token_id"], hf["num_attention_heads"]
    mask = (torch.arange(T)[None, :] < lengths[:, None]).long()
    pos = torch.cumsum(mask, 1) * mask + pad                              # create_position_ids_from_input_ids
    e = "embeddings."
    x = W[e + "word_embeddings.weight"][ids] + W[e + "token_type_embeddings.weight"][0] + W[e + "position_embeddings.weight"][pos]
    x = layer_norm(x, W[e + "LayerNorm.weight"], W[e + "LayerNorm.bias"], eps)
    for i in range(hf["num_hidden_layers"]):
        l = f"encoder.layer.{i}."
        a = l + "attention.self."
        ctx = attention(lin(x, a + "query"), lin(x, a + "key"), lin(x, a + "value"), lengths, heads)
        x = layer_norm(lin(ctx, l + "attention.output.dense") + x, W[l + "attention.output.LayerNorm.weight"],
                       W[l + "attention.output.LayerNorm.bias"], eps)
        up = gelu_erf(lin(x, l + "intermediate.dense"))
        x = layer_norm(lin(up, l + "output.dense") + x, W[l + "output.LayerNorm.weight"], W[l + "output.LayerNorm.bias"], eps)
    return x


def pool_tail(hidden, lengths, max_length, bert_norm):
    """reference encoder.py:50-70 on [B, T, H]: words_embs [B, H, max_length] (zero at padding and beyond T), sent_embs [B, H],
    mask [B, max_length] (True at padding)"""
    B, T, H = hidden.shape
    attn = (torch.arange(T)[None, :] < torch.as_tensor(lengths)[:, None])
    emb = hidden * attn[:, :, None].to(hidden.dtype)
    sent = emb.sum(1) / attn[:, :, None].sum(1).to(hidden.dtype)
    if bert_norm:
        sent = torch.nn.functional.normalize(sent, p=2, dim=1)
    words = torch.zeros(B, H, max_length, dtype=hidden.dtype)
    words[:, :, :T] = emb.transpose(1, 2)
    mask = torch.ones(B, max_length, dtype=torch.bool)
    mask[:, :T] = ~attn
    return words, sent, mask


def encode(w, hf, input_ids, lengths, max_length, bert_norm, gemm_fmt=None):
    return pool_tail(hidden_states(w, hf, input_ids, lengths, gemm_fmt), lengths, max_length, bert_norm)


def random_batch(hf, lengths, T, seed):
    """int64 [B, T]: <s> tokens </s> then the pad id, ordinary tokens drawn from the ids above the specials"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((len(lengths), T), hf["pad_token_id"], dtype=torch.int64)
    for b, n in enumerate(lengths):
        ids[b, 0], ids[b, n - 1] = hf["bos_token_id"], hf["eos_token_id"]
        ids[b, 1:n - 1] = torch.randint(4, hf["vocab_size"], (n - 2,), generator=g)
    return ids, torch.tensor(lengths, dtype=torch.int64)
