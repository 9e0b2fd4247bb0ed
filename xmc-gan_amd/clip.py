"""CLIPScore on the device: the two towers of a Hugging Face ``CLIPModel`` directory (CLIP ViT-B/32) and the per-image cosine.

``CLIPScorer(model_dir, device)`` reads ``config.json``, ``model.safetensors`` or ``pytorch_model.bin``, ``tokenizer.json`` and, when it is
there, ``preprocessor_config.json`` -- no third-party model code -- and runs both forwards on the MI355X in f32 whatever
``ops.set_precision`` says, like ``InceptionFID``: the f32 MFMA GEMMs of the 1x1 convolution path (bias and residual in their epilogue),
``ops.add_layernorm`` / ``ops.attention_short`` / ``ops.bias_gelu`` of the sentence encoder, and the kernels of csrc/clip.hip (Pillow's
integer bicubic resize with the crop, the normalisation and the patch order in its second pass; the two embedding blocks; causal
attention; QuickGELU; the pooled-row LayerNorm; the cosine).  No atomics: the same inputs give the same bytes.

By default the text tower's context is ``min(max_position_embeddings, 64)`` tokens, the longest sequence the short attention kernels take.
Attention is causal and the pooled row is the caption's EOS, so nothing after the EOS reaches a feature: a caption of at most 62 BPE tokens
gets the feature it gets at CLIP's own context of 77; a longer one is truncated earlier than upstream would (counted in ``n_truncated``).

``CLIPScorer(model_dir, device, max_tokens=N)`` with N in (64, 1024] opts into ``ops.attention_long`` (csrc/attention_long.hip: f32 MFMA
attention with K and V streamed through LDS): a vision tower of up to N tokens is accepted (ViT-B/16 has 197, L/14 257, L/14 at 336 px
577) and the context is ``min(max_position_embeddings, N)``, CLIP's own 77, so that truncation and ``n_truncated`` follow upstream.  Each
tower keeps ONE attention kernel, chosen at construction by its longest sequence (``tokens`` / ``context``): at most 64 the short kernels,
beyond that ``attention_long`` for every call, so a caption's bytes never depend on the longest caption of its batch.
"""
import json
import os

import torch

from . import hfdir
from . import lib as L
from . import ops

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
MAX_CONTEXT = ops.ATTENTION_MAX_T              # the attention kernels' longest sequence
_FILES = "config.json, model.safetensors or pytorch_model.bin, tokenizer.json [, preprocessor_config.json]"


class _Tower:
    """the sizes of one tower, from its half of config.json"""

    def __init__(self, name, hf, cj):
        self.name = name
        try:
            self.width, self.layers = int(hf["hidden_size"]), int(hf["num_hidden_layers"])
            self.heads, self.ffn = int(hf["num_attention_heads"]), int(hf["intermediate_size"])
        except KeyError as e:
            raise ImportError(f"CLIPScorer: {name} of {cj} lacks {e.args[0]!r}") from e
        self.act = hf.get("hidden_act", "quick_gelu")
        self.eps = float(hf.get("layer_norm_eps", 1e-5))
        W = self.width
        if self.heads * 64 != W:
            raise NotImplementedError(f"CLIPScorer: the kernels are built for head dimension 64; {name} has width {W} and {self.heads} heads")
        if W % 64 or W > ops.LN_MAX_WIDTH or self.ffn % 8:
            raise NotImplementedError(f"CLIPScorer: the kernels are built for a width that is a multiple of 64 and <= 1024 and "
                                      f"intermediate_size % 8 == 0; {name} has width {W}, intermediate_size {self.ffn}")
        if self.act not in ("quick_gelu", "gelu"):
            raise NotImplementedError(f"CLIPScorer: {name} has hidden_act={self.act!r}; the forward is built for 'quick_gelu' and 'gelu'")
        self.geoms = (ops.ConvGeom(W, 3 * W, 1, 1, 0), ops.ConvGeom(W, W, 1, 1, 0), ops.ConvGeom(W, self.ffn, 1, 1, 0),
                      ops.ConvGeom(self.ffn, W, 1, 1, 0))


class CLIPScorer:
    """``encode_images`` / ``tokenize`` / ``encode_text_ids`` / ``encode_text`` / ``score``; ``n_truncated`` counts the captions
    ``tokenize`` cut to the context."""

    def __init__(self, model_dir, device=None, max_tokens=MAX_CONTEXT):
        if isinstance(max_tokens, bool) or not isinstance(max_tokens, int) or not MAX_CONTEXT <= max_tokens <= ops.ATTENTION_LONG_MAX_T:
            raise ValueError(f"CLIPScorer: max_tokens must be an integer in [{MAX_CONTEXT}, {ops.ATTENTION_LONG_MAX_T}], got {max_tokens!r}")
        self.max_tokens = max_tokens
        if not model_dir or not os.path.isdir(model_dir):
            raise ImportError(f"CLIPScorer needs a Hugging Face CLIPModel directory ({_FILES}; e.g. a copy of openai/clip-vit-base-patch32); "
                              f"{model_dir!r} is not a directory")
        cj = os.path.join(model_dir, "config.json")
        if not os.path.isfile(cj):
            raise ImportError(f"CLIPScorer: {model_dir} holds no config.json")
        with open(cj) as f:
            hf = json.load(f)
        for part in ("vision_config", "text_config", "projection_dim"):
            if part not in hf:
                raise ImportError(f"CLIPScorer: {cj} lacks {part!r} (a CLIPModel's config.json is expected)")
        self.model_dir, self.device = model_dir, torch.device(device if device is not None else "cpu")
        self.name = os.path.basename(os.path.normpath(model_dir))
        vc, tc = hf["vision_config"], hf["text_config"]
        self.vision, self.text = _Tower("vision_config", vc, cj), _Tower("text_config", tc, cj)
        self.dim = int(hf["projection_dim"])
        if self.dim % 8:
            raise NotImplementedError(f"CLIPScorer: the GEMMs are built for projection_dim % 8 == 0, got {self.dim}")
        try:
            self.image_size, self.patch = int(vc["image_size"]), int(vc["patch_size"])
            self.vocab, self.npos = int(tc["vocab_size"]), int(tc["max_position_embeddings"])
        except KeyError as e:
            raise ImportError(f"CLIPScorer: {cj} lacks {e.args[0]!r}") from e
        if self.image_size % self.patch:
            raise ValueError(f"CLIPScorer: image_size {self.image_size} is no multiple of patch_size {self.patch}")
        self.grid = self.image_size // self.patch
        self.tokens = self.grid * self.grid + 1
        if self.tokens > max_tokens and max_tokens > MAX_CONTEXT:
            raise NotImplementedError(f"CLIPScorer: image_size {self.image_size} / patch_size {self.patch} gives {self.tokens} tokens, more than "
                                      f"max_tokens={max_tokens} (--clip_max_tokens) admits; {self.tokens} or more, up to "
                                      f"{ops.ATTENTION_LONG_MAX_T}, takes this model")
        if self.tokens > MAX_CONTEXT and max_tokens == MAX_CONTEXT:
            raise NotImplementedError(f"CLIPScorer: the attention kernel takes at most {MAX_CONTEXT} tokens; image_size {self.image_size} / "
                                      f"patch_size {self.patch} gives {self.tokens} (ViT-B/32 at 224 has 50; B/16 and L/14 are not built)")
        self.bos_id, self.eos_id = int(tc.get("bos_token_id", 49406)), int(tc.get("eos_token_id", 49407))
        self.pad_id = int(tc["pad_token_id"]) if tc.get("pad_token_id") is not None else 0
        self.context = min(self.npos, max_tokens)
        # one attention kernel per tower, by its longest sequence: a sample's bytes do not depend on its batch
        self.vision.long, self.text.long = self.tokens > MAX_CONTEXT, self.context > MAX_CONTEXT
        self.n_truncated = 0
        self.image_batch = 256
        self._tokenizer = None
        self._read_preprocessor()
        self._w = self._assemble(hfdir.read_weights(model_dir, "CLIPScorer"), cj)
        self._lut = None
        self.g_patch = ops.ConvGeom(3 * self.patch * self.patch, self.vision.width, 1, 1, 0)
        self.g_vproj, self.g_tproj = ops.ConvGeom(self.vision.width, self.dim, 1, 1, 0), ops.ConvGeom(self.text.width, self.dim, 1, 1, 0)

    # ------------------------------------------------------------------ loading
    def _read_preprocessor(self):
        pj = os.path.join(self.model_dir, "preprocessor_config.json")
        pc = {}
        if os.path.isfile(pj):
            with open(pj) as f:
                pc = json.load(f)
        if int(pc.get("resample", 3)) != 3:
            raise NotImplementedError(f"CLIPScorer: {pj} has resample={pc['resample']}; the resize kernel is Pillow's bicubic (3)")
        self.mean = tuple(float(v) for v in pc.get("image_mean", CLIP_MEAN))
        self.std = tuple(float(v) for v in pc.get("image_std", CLIP_STD))
        size, crop = pc.get("size", self.image_size), pc.get("crop_size", self.image_size)
        self.short = int(size.get("shortest_edge", size.get("height", self.image_size))) if isinstance(size, dict) else int(size)
        self.crop = int(crop.get("height", self.image_size)) if isinstance(crop, dict) else int(crop)
        if len(self.mean) != 3 or len(self.std) != 3 or self.crop != self.image_size or self.short < self.crop:
            raise ValueError(f"CLIPScorer: {pj} (three-channel mean / std, crop_size == image_size {self.image_size} <= size) does not fit: "
                             f"mean {self.mean}, std {self.std}, size {self.short}, crop_size {self.crop}")

    def _assemble(self, sd, cj):
        """the tensors the forwards read, as frozen f32 Parameters on the device (so that their packed copies are cached): q, k and v of a
        layer as one [3W, W] weight, the patch embedding as [W, 3 P P]"""
        w = {}
        take, frozen = hfdir.weight_access(sd, "CLIPScorer", self.model_dir, cj, self.device)
        V, T, P = self.vision, self.text, self.patch
        v, t = "vision_model.", "text_model."
        w["v.cls"] = frozen(take(v + "embeddings.class_embedding", (V.width,)))
        w["v.patch"] = frozen(take(v + "embeddings.patch_embedding.weight", (V.width, 3, P, P)).reshape(V.width, 3 * P * P))
        w["v.pos"] = frozen(take(v + "embeddings.position_embedding.weight", (self.tokens, V.width)))
        w["t.tok"] = frozen(take(t + "embeddings.token_embedding.weight", (self.vocab, T.width)))
        w["t.pos"] = frozen(take(t + "embeddings.position_embedding.weight", (self.npos, T.width)))
        for name, key, W in (("v.pre", v + "pre_layrnorm", V.width), ("v.post", v + "post_layernorm", V.width),
                             ("t.final", t + "final_layer_norm", T.width)):
            w[name + "g"], w[name + "b"] = frozen(take(key + ".weight", (W,))), frozen(take(key + ".bias", (W,)))
        w["v.proj"] = frozen(take("visual_projection.weight", (self.dim, V.width)))
        w["t.proj"] = frozen(take("text_projection.weight", (self.dim, T.width)))
        for pre, root, tw in (("v", v, V), ("t", t, T)):
            W, F = tw.width, tw.ffn
            for i in range(tw.layers):
                l = f"{root}encoder.layers.{i}."
                a = l + "self_attn."
                w[f"{pre}.{i}.wqkv"] = frozen(torch.cat([take(a + n + "_proj.weight", (W, W)) for n in "qkv"], 0))
                w[f"{pre}.{i}.bqkv"] = frozen(torch.cat([take(a + n + "_proj.bias", (W,)) for n in "qkv"], 0))
                for name, key, shape in (("wo", "self_attn.out_proj", (W, W)), ("w1", "mlp.fc1", (F, W)), ("w2", "mlp.fc2", (W, F))):
                    w[f"{pre}.{i}.{name}"] = frozen(take(l + key + ".weight", shape))
                    w[f"{pre}.{i}.b{name[1:]}"] = frozen(take(l + key + ".bias", shape[:1]))
                for name, key in (("ln1", "layer_norm1"), ("ln2", "layer_norm2")):
                    w[f"{pre}.{i}.{name}g"], w[f"{pre}.{i}.{name}b"] = frozen(take(l + key + ".weight", (W,))), frozen(take(l + key + ".bias", (W,)))
        return w

    # ------------------------------------------------------------------ host side: sentences -> token ids
    def tokenizer(self):
        if self._tokenizer is None:
            self._tokenizer = hfdir.load_tokenizer(
                self.model_dir, "CLIPScorer", ("",), "CLIPScorer.tokenize uses the `tokenizers` package, which is not importable here; call "
                "encode_text_ids(ids, lens) with ids tokenized elsewhere")
        return self._tokenizer

    def tokenize(self, sentences):
        """sentences -> (int64 [B, T] right-padded with the pad id, int64 [B] lengths), T the longest row: the directory's tokenizer with
        its own normaliser and pre-tokeniser, BOS ... EOS around each, truncated to ``context`` tokens INCLUDING both (EOS stays last)"""
        encs = self.tokenizer().encode_batch([str(s) for s in sentences], add_special_tokens=False)
        rows = []
        for e in encs:
            body = list(e.ids)
            self.n_truncated += len(body) > self.context - 2
            rows.append([self.bos_id] + body[:self.context - 2] + [self.eos_id])
        lens = torch.tensor([len(r) for r in rows], dtype=torch.int64)
        ids = torch.full((len(rows), int(lens.max()) if rows else 0), self.pad_id, dtype=torch.int64)
        for i, r in enumerate(rows):
            ids[i, :len(r)] = torch.tensor(r, dtype=torch.int64)
        return ids, lens

    # ------------------------------------------------------------------ device side
    @staticmethod
    def _gemm(x, w, b, geom, res=None):
        M = x.shape[0]
        y = ops._conv_fwd_raw(x.view(M, 1, 1, x.shape[1]), w, b, geom, L.ACT_NONE, torch.float32,
                              res=None if res is None else res.view(M, 1, 1, res.shape[1]))
        return y.view(M, -1)

    def _layers(self, x, pre, tw, B, T, causal):
        """the pre-LayerNorm transformer layers of one tower over the residual stream x f32 [B*T, W]"""
        w = self._w
        g_qkv, g_o, g_up, g_down = tw.geoms
        full = None if causal or tw.long else torch.full((B,), T, dtype=torch.int32, device=x.device)
        for i in range(tw.layers):
            g = lambda n: w[f"{pre}.{i}.{n}"]      # noqa: E731
            h, _ = ops.add_layernorm(x, None, g("ln1g"), g("ln1b"), tw.eps)
            qkv = self._gemm(h, g("wqkv"), g("bqkv"), g_qkv)
            if tw.long:
                ctx = ops.attention_long(qkv, None, B, T, tw.heads, causal=causal)
            else:
                ctx = ops.attention_causal(qkv, B, T, tw.heads) if causal else ops.attention_short(qkv, full, B, T, tw.heads)
            x = self._gemm(ctx, g("wo"), g("bo"), g_o, res=x)
            h, _ = ops.add_layernorm(x, None, g("ln2g"), g("ln2b"), tw.eps)
            up = self._gemm(h, g("w1"), None, g_up)
            act = ops.bias_quick_gelu(up, g("b1")) if tw.act == "quick_gelu" else ops.bias_gelu(up, g("b1"))
            x = self._gemm(act, g("w2"), g("b2"), g_down, res=x)
        return x

    def lut(self):
        """f32 [3, 256] on the device: (v / 255 - mean_c) / std_c, computed in f64"""
        if self._lut is None:
            v = torch.arange(256, dtype=torch.float64)[None, :] / 255.0
            mean, std = (torch.tensor(t, dtype=torch.float64)[:, None] for t in (self.mean, self.std))
            self._lut = ((v - mean) / std).to(torch.float32).to(self.device).contiguous()
        return self._lut

    @torch.no_grad()
    def encode_images(self, u8):
        """uint8 [N, H, W, 3] on the device, all of one size -> image features f32 [N, D] (not normalised)"""
        if u8.dim() != 4 or u8.shape[3] != 3 or u8.dtype != torch.uint8:
            raise ValueError(f"CLIPScorer.encode_images: uint8 images [N,H,W,3] expected, got {u8.dtype} {tuple(u8.shape)}")
        if not u8.is_cuda:
            raise RuntimeError("CLIPScorer.encode_images: CPU tensors are not supported (no CPU fallback)")
        w, V, GG = self._w, self.vision, self.grid * self.grid
        u8 = u8.contiguous()
        outs = []
        for lo in range(0, u8.shape[0], self.image_batch):
            part = u8[lo:lo + self.image_batch]
            N = part.shape[0]
            rows = ops.clip_patch_rows(part, self.short, self.crop, self.patch, self.lut())
            emb = self._gemm(rows, w["v.patch"], None, self.g_patch)
            x = ops.clip_vision_embed(emb, w["v.cls"], w["v.pos"], w["v.preg"], w["v.preb"], V.eps)
            x = self._layers(x, "v", V, N, GG + 1, causal=False)
            pooled = ops.clip_pool_ln(x, torch.zeros(N, dtype=torch.int32, device=x.device), GG + 1, w["v.postg"], w["v.postb"], V.eps)
            outs.append(self._gemm(pooled, w["v.proj"], None, self.g_vproj))
        return outs[0] if len(outs) == 1 else torch.cat(outs, 0)

    @torch.no_grad()
    def encode_text_ids(self, ids, lens):
        """ids int64 [B, T <= context] (BOS ... EOS, then anything), lens [B] (tokens including both specials) -> text features f32 [B, D]"""
        ids, lens = torch.as_tensor(ids), torch.as_tensor(lens)
        if ids.dim() != 2 or not 1 <= ids.size(1) <= self.context or lens.numel() != ids.size(0):
            raise ValueError(f"ids must be [B, T <= {self.context}] with one length per row, got {tuple(ids.shape)} / {tuple(lens.shape)}")
        B, T = ids.shape
        if not ids.is_cuda:           # host tensors: validate for free
            if int(lens.min()) < 1 or int(lens.max()) > T:
                raise ValueError("caption lengths must lie in [1, T]")
            if int(ids.min()) < 0 or int(ids.max()) >= self.vocab:
                raise IndexError("token id outside [0, vocab_size)")
        if self.device.type != "cuda":
            raise RuntimeError("CLIPScorer.encode_text_ids: the scorer was loaded on the CPU (no CPU fallback)")
        w, tw = self._w, self.text
        ids = ids.to(self.device, torch.int64).contiguous()
        eos = (lens.to(self.device, torch.int64) - 1).to(torch.int32).contiguous()
        x = ops.clip_text_embed(ids, w["t.tok"], w["t.pos"])
        x = self._layers(x, "t", tw, B, T, causal=True)
        pooled = ops.clip_pool_ln(x, eos, T, w["t.finalg"], w["t.finalb"], tw.eps)
        return self._gemm(pooled, w["t.proj"], None, self.g_tproj)

    def encode_text(self, sentences):
        ids, lens = self.tokenize(sentences)
        return self.encode_text_ids(ids, lens)

    @torch.no_grad()
    def score(self, img_feats, txt_feats, caption_of_image=None):
        """f32 [N]: the cosine of every image's feature row and its caption's (row ``caption_of_image[n]`` of ``txt_feats``, or row n)"""
        if caption_of_image is not None:
            caption_of_image = torch.as_tensor(caption_of_image)
            if not caption_of_image.is_cuda and caption_of_image.numel() and \
                    (int(caption_of_image.min()) < 0 or int(caption_of_image.max()) >= txt_feats.shape[0]):
                raise IndexError("caption_of_image outside the caption rows")
            caption_of_image = caption_of_image.to(img_feats.device, torch.int32).contiguous()
        return ops.clip_cosine(img_feats.contiguous(), txt_feats.contiguous(), caption_of_image)



class CLIPScoreStats:
    """CLIPScore of the generated images of an evaluation: ``update`` scores a batch against its captions and keeps the per-image cosines on
    the device, ``finalize`` reduces them in f64."""

    def __init__(self, scorer):
        self.scorer, self._cos, self.n_truncated = scorer, [], 0

    def update(self, u8, captions, caption_of_image=None):
        """uint8 [N,H,W,3] images and their caption strings: one per image, or fewer with ``caption_of_image`` [N] naming each image's.
        Each distinct caption of the batch is encoded once."""
        captions, N = [str(c) for c in captions], u8.shape[0]
        rows = list(range(N)) if caption_of_image is None else [int(i) for i in torch.as_tensor(caption_of_image).tolist()]
        if len(rows) != N or (caption_of_image is None and len(captions) != N) or any(not 0 <= r < len(captions) for r in rows):
            raise IndexError(f"CLIPScore: {N} images, {len(captions)} captions and caption_of_image {rows[:8]}... do not pair up")
        distinct = {}
        which = [distinct.setdefault(captions[r], len(distinct)) for r in rows]
        before = self.scorer.n_truncated
        txt = self.scorer.encode_text(list(distinct))
        self.n_truncated += self.scorer.n_truncated - before
        img = self.scorer.encode_images(u8)
        self._cos.append(self.scorer.score(img, txt, torch.tensor(which, dtype=torch.int32)))

    def finalize(self):
        """dict(clip_score, std, cosine, n, n_truncated, model): the mean and (population) standard deviation of max(100 cos, 0) over the
        images -- the torchmetrics convention; Hessel et al.'s 2.5 max(cos, 0) is 0.025 times it -- and the mean raw cosine, in f64"""
        if not self._cos:
            raise ValueError("no caption text reached the metric")
        cos = torch.cat([c.detach().to("cpu", torch.float64) for c in self._cos])
        per = (100.0 * cos).clamp_min(0.0)
        return dict(clip_score=float(per.mean()), std=float(per.std(unbiased=False)), cosine=float(cos.mean()), n=int(cos.numel()),
                    n_truncated=int(self.n_truncated), model=self.scorer.name)
