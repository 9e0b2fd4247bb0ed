"""Frozen encoders: the reference's two text encoders with its class names and call signature (model/encoder.py), and the image half
of the DAMSM pair, which the reference does not have (``CNN_ENCODER``, AttnGAN's, for R-precision).

``RNN_ENCODER`` (the DAMSM caption encoder, encoder.py:73-153) holds an ``nn.Embedding`` and an ``nn.LSTM`` as parameter
containers -- ``state_dict()`` keys and shapes are upstream's, so ``text_encoder100.pth`` loads unchanged -- and runs
its forward on the MI355X kernels: embedding gather, one f32 MFMA GEMM for the input projections of every token and
both directions, and the per-sample LSTM recurrence kernel.  Forward only: the reference freezes the encoder and
puts it in eval mode (train_gan.py:464-468).

``SBERT_ENCODER`` (encoder.py:24-70) wraps ``sentence_transformers.SentenceTransformer('stsb-roberta-base')`` upstream: a
byte-level BPE tokenizer, a frozen 12-layer RoBERTa-base forward and a masked mean pooling.  Here it reads a model directory
the user supplies (``model_dir`` / ``XMC_SBERT_DIR``: config.json, weights, tokenizer files -- no third-party model code) and
runs the forward on the MI355X: four MFMA GEMMs per layer through ``ops.linear`` and the kernels of csrc/transformer.hip
(embedding sum + LayerNorm, fused short-sequence attention, bias + erf GELU, residual + LayerNorm, the pooling tail).
Without a model directory constructing it fails loudly (ImportError), as before.

``CNN_ENCODER`` (AttnGAN model.py, not in the reference) is torchvision's Inception-v3 up to ``Mixed_7c`` plus two projections, with
AttnGAN's ``state_dict()`` keys so that ``image_encoder100.pth`` loads unchanged.  Its forward is the f32 Inception trunk of
``xmc_gan_amd.fid`` in its torchvision variant, behind a float (or uint8) bilinear front end.
"""
import json
import os

import torch
import torch.nn as nn

from xmc_gan_amd import hfdir
from xmc_gan_amd import lib as _L
from xmc_gan_amd import ops


class RNN_ENCODER(nn.Module):
    def __init__(self, cfg):
        super(RNN_ENCODER, self).__init__()
        self.n_steps = cfg.TEXT.MAX_LENGTH
        self.ntoken = cfg.TEXT.VOCA_SIZE
        self.ninput = 300
        self.drop_prob = 0.5
        self.nlayers = 1
        self.bidirectional = True
        self.rnn_type = cfg.TEXT.RNN_TYPE
        self.num_directions = 2
        self.nhidden = cfg.TEXT.EMBEDDING_DIM // self.num_directions
        if self.rnn_type not in ('LSTM', 'GRU'):
            raise NotImplementedError(f"TEXT.RNN_TYPE={self.rnn_type!r} (encoder.py:103)")
        self.ngates = 4 if self.rnn_type == 'LSTM' else 3
        self.encoder = nn.Embedding(self.ntoken, self.ninput)
        self.drop = nn.Dropout(self.drop_prob)
        # dropout= is a no-op for a single layer; left out to spare the construction-time warning (same parameters)
        rnn = nn.LSTM if self.rnn_type == 'LSTM' else nn.GRU               # encoder.py:95-102
        self.rnn = rnn(self.ninput, self.nhidden, self.nlayers, batch_first=True, bidirectional=True)
        self.encoder.weight.data.uniform_(-0.1, 0.1)                       # _init_weights (encoder.py:106-108)
        self.geom = ops.ConvGeom(self.ninput, 2 * self.ngates * self.nhidden, 1, 1, 0)
        self._packed = None

    def _weights(self):
        """[W_ih_fwd; W_ih_rev] (2*G*H, 300), input-side biases (2*G*H), [W_hh_fwd, W_hh_rev] (2, G*H, H) [, GRU: b_hn (2, H)];
        G = 4 gate rows (LSTM) or 3 (GRU); rebuilt when a parameter changes (load_state_dict, .to()).
        LSTM: the two bias vectors add up front.  GRU: b_hh of the r and z rows likewise, but the candidate gate is
        tanh(W_in x + b_in + r * (W_hn h + b_hn)), so its hidden bias stays with the recurrence."""
        r = self.rnn
        ps = (r.weight_ih_l0, r.weight_ih_l0_reverse, r.weight_hh_l0, r.weight_hh_l0_reverse,
              r.bias_ih_l0, r.bias_ih_l0_reverse, r.bias_hh_l0, r.bias_hh_l0_reverse)
        key = tuple((p.data_ptr(), p._version) for p in ps)
        if self._packed is None or self._packed[0] != key:
            with torch.no_grad():
                w_ih = torch.cat((ps[0], ps[1]), 0).float().contiguous()
                w_hh = torch.stack((ps[2], ps[3]), 0).float().contiguous()
                if self.rnn_type == 'LSTM':
                    bias = torch.cat((ps[4] + ps[6], ps[5] + ps[7]), 0).float().contiguous()
                    extra = ()
                else:
                    H = self.nhidden
                    keep = torch.cat((torch.ones(2 * H), torch.zeros(H))).to(ps[6])            # b_hr, b_hz join; b_hn does not
                    bias = torch.cat((ps[4] + ps[6] * keep, ps[5] + ps[7] * keep), 0).float().contiguous()
                    extra = (torch.stack((ps[6][2 * H:], ps[7][2 * H:]), 0).float().contiguous(),)
            self._packed = (key, w_ih, bias, w_hh) + extra
        return self._packed[1:]

    def forward(self, caps, cap_lens, **kwargs):
        """caps int64 [B, n_steps] (0 = padding), cap_lens [B] -> words_embs [B, E, n_steps], sent_embs [B, E],
        mask [B, n_steps] (True at padding), all on the encoder's device."""
        if self.training:
            raise NotImplementedError("RNN_ENCODER runs frozen in eval mode (train_gan.py:466-468); the dropout of "
                                      "training mode (encoder.py:132) is not built")
        dev = self.encoder.weight.device
        caps, cap_lens = torch.as_tensor(caps), torch.as_tensor(cap_lens)
        if caps.dim() != 2 or caps.size(1) != self.n_steps:
            raise ValueError(f"caps must be [B, {self.n_steps}] token ids, got {tuple(caps.shape)}")
        if not caps.is_cuda:      # loader output: validate on the host for free (pack_padded_sequence raises upstream)
            if int(cap_lens.min()) < 1 or int(cap_lens.max()) > self.n_steps:
                raise ValueError("caption lengths must lie in [1, TEXT.MAX_LENGTH]")
            if int(caps.min()) < 0 or int(caps.max()) >= self.ntoken:
                raise IndexError("token id outside [0, TEXT.VOCA_SIZE)")
        caps = caps.to(dev, torch.int64, non_blocking=True)
        lens = cap_lens.to(dev, torch.int32, non_blocking=True).contiguous()
        w_ih, bias, w_hh, *extra = self._weights()
        B, T = caps.shape
        emb = ops.embedding(caps, self.encoder.weight)                                     # [B, T, 300]
        xproj = ops.linear(emb.view(B * T, self.ninput), w_ih, bias, self.geom, out_dtype=torch.float32)
        xproj = xproj.view(B, T, 2, self.ngates * self.nhidden)
        if self.rnn_type == 'LSTM':
            words_embs, sent_embs = ops.lstm_bidir(xproj, w_hh, lens, T)
        else:
            words_embs, sent_embs = ops.gru_bidir(xproj, w_hh, extra[0], lens, T)
        mask = (caps == 0)
        return words_embs, sent_embs, mask


_SBERT_SUBDIRS = ("", "0_Transformer")          # the directory itself; the older sentence-transformers layout
_SBERT_DROP = ("pooler.", "lm_head.", "classifier.", "embeddings.position_ids")


def _sbert_read_weights(model_dir):
    """{Hugging Face key without the 'roberta.' prefix: tensor}; pooler / LM head keys dropped"""
    sd = hfdir.read_weights(model_dir, "SBERT_ENCODER", _SBERT_SUBDIRS, " (looked in the directory and in 0_Transformer/)")
    out = {}
    for k, v in sd.items():
        k = k[len("roberta."):] if k.startswith("roberta.") else k
        if not k.startswith(_SBERT_DROP):
            out[k] = v
    return out


class SBERT_ENCODER(nn.Module):
    """``SBERT_ENCODER(cfg, model_dir=None)``: the reference's call signature, ``forward(sents, sent_lens)`` ->
    ``words_embs [B, H, MAX_LENGTH]``, ``sent_embs [B, H]``, ``mask [B, MAX_LENGTH]`` (True at padding).

    One difference from upstream: ``words_embs`` and ``mask`` are always ``TEXT.MAX_LENGTH`` wide instead of cut to the batch's
    longest sentence -- a static shape for the replayed iteration; the extra columns are zero and masked.
    The weights are frozen tensors outside ``state_dict()`` (the reference never loads or saves this encoder's state); they move
    with ``.to(device)``."""

    def __init__(self, cfg, model_dir=None):
        super(SBERT_ENCODER, self).__init__()
        model_dir = model_dir or os.environ.get("XMC_SBERT_DIR", "")
        if not model_dir:
            raise ImportError(
                "SBERT_ENCODER needs a RoBERTa model directory (config.json, model.safetensors or pytorch_model.bin, tokenizer.json or "
                "vocab.json + merges.txt; e.g. a download of sentence-transformers/stsb-roberta-base): pass model_dir= / --sbert_dir or "
                "set XMC_SBERT_DIR.  None is given.  Use a TEXT.ENCODER_NAME: 'RNN' preset or --synthetic otherwise.")
        if not os.path.isdir(model_dir):
            raise ImportError(f"SBERT_ENCODER: the model directory {model_dir} does not exist")
        cj = hfdir.find(model_dir, ("config.json",), _SBERT_SUBDIRS)
        if cj is None:
            raise ImportError(f"SBERT_ENCODER: {model_dir} holds no config.json (looked in the directory and in 0_Transformer/)")
        with open(cj) as f:
            hf = json.load(f)
        for key, want in (("model_type", "roberta"), ("hidden_act", "gelu"), ("position_embedding_type", "absolute")):
            got = hf.get(key, "absolute" if key == "position_embedding_type" else None)
            if got != want:
                raise NotImplementedError(f"SBERT_ENCODER: {cj} has {key}={got!r}; the forward is built for {want!r}")
        self.bert_norm = bool(cfg.TEXT.BERT_NORM)
        self.pooling_mode = cfg.TEXT.POOLING_MODE
        self.max_seq_length = int(cfg.TEXT.MAX_LENGTH)
        if self.pooling_mode != 'MEAN':
            raise NotImplementedError(f"TEXT.POOLING_MODE={self.pooling_mode!r} (encoder.py:20-21)")
        H, self.nlayers = int(hf["hidden_size"]), int(hf["num_hidden_layers"])
        self.hidden, self.heads, self.ffn = H, int(hf["num_attention_heads"]), int(hf["intermediate_size"])
        self.eps = float(hf.get("layer_norm_eps", 1e-5))
        self.pad_id, self.bos_id, self.eos_id = (int(hf.get(k, d)) for k, d in (("pad_token_id", 1), ("bos_token_id", 0), ("eos_token_id", 2)))
        self.vocab, self.npos = int(hf["vocab_size"]), int(hf["max_position_embeddings"])
        if H != cfg.TEXT.EMBEDDING_DIM:
            raise ValueError(f"SBERT_ENCODER: {cj} has hidden_size {H}, the preset's TEXT.EMBEDDING_DIM is {cfg.TEXT.EMBEDDING_DIM}")
        if self.heads * 64 != H or H > ops.LN_MAX_WIDTH or self.ffn % 8 or self.max_seq_length > ops.ATTENTION_MAX_T:
            raise NotImplementedError(f"SBERT_ENCODER: the kernels are built for head dimension 64, hidden_size <= 1024, intermediate_size % 8 "
                                      f"== 0 and TEXT.MAX_LENGTH <= 64 (got hidden {H}, {self.heads} heads, FFN {self.ffn}, MAX_LENGTH {self.max_seq_length})")
        if self.max_seq_length + self.pad_id + 1 > self.npos:
            raise ValueError(f"SBERT_ENCODER: max_position_embeddings {self.npos} is too small for TEXT.MAX_LENGTH {self.max_seq_length}")
        self.model_dir = model_dir
        self._tokenizer = None
        self._w = self._assemble(_sbert_read_weights(model_dir), cj)
        self.geom_qkv, self.geom_o = ops.ConvGeom(H, 3 * H, 1, 1, 0), ops.ConvGeom(H, H, 1, 1, 0)
        self.geom_up, self.geom_down = ops.ConvGeom(H, self.ffn, 1, 1, 0), ops.ConvGeom(self.ffn, H, 1, 1, 0)
        self.eval()

    def _assemble(self, sd, cj):
        """the tensors the forward reads, as frozen f32 Parameters (so that `ops.linear` caches their packed copies until one changes):
        Q, K, V of a layer as one [3H, H] weight"""
        H, F = self.hidden, self.ffn
        w = {}
        take, frozen = hfdir.weight_access(sd, "SBERT_ENCODER", self.model_dir, cj)
        e = "embeddings."
        w["word"] = frozen(take(e + "word_embeddings.weight", (self.vocab, H)))
        w["pos"] = frozen(take(e + "position_embeddings.weight", (self.npos, H)))
        tt = sd.get(e + "token_type_embeddings.weight")
        if tt is None or tt.dim() != 2 or tt.shape[1] != H:
            raise ImportError(f"SBERT_ENCODER: the weights in {self.model_dir} lack {e}token_type_embeddings.weight [*, {H}]")
        w["type0"] = frozen(tt[0].detach().float())
        w["emb_g"], w["emb_b"] = frozen(take(e + "LayerNorm.weight", (H,))), frozen(take(e + "LayerNorm.bias", (H,)))
        for i in range(self.nlayers):
            l = f"encoder.layer.{i}."
            a = l + "attention.self."
            w[f"{i}.wqkv"] = frozen(torch.cat([take(a + n + ".weight", (H, H)) for n in ("query", "key", "value")], 0))
            w[f"{i}.bqkv"] = frozen(torch.cat([take(a + n + ".bias", (H,)) for n in ("query", "key", "value")], 0))
            for name, key, shape in (("wo", "attention.output.dense", (H, H)), ("w1", "intermediate.dense", (F, H)), ("w2", "output.dense", (H, F))):
                w[f"{i}.{name}"] = frozen(take(l + key + ".weight", shape))
                w[f"{i}.b{name[1:]}"] = frozen(take(l + key + ".bias", shape[:1]))
            for name, key in (("ln1", "attention.output.LayerNorm"), ("ln2", "output.LayerNorm")):
                w[f"{i}.{name}g"], w[f"{i}.{name}b"] = frozen(take(l + key + ".weight", (H,))), frozen(take(l + key + ".bias", (H,)))
        return w

    def _apply(self, fn, recurse=True):
        super(SBERT_ENCODER, self)._apply(fn, recurse)
        with torch.no_grad():
            self._w = {k: nn.Parameter(fn(v.data).float().contiguous(), requires_grad=False) for k, v in self._w.items()}
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("SBERT_ENCODER runs frozen in eval mode (encoder.py:36,40); fine-tuning it is not built")
        return super(SBERT_ENCODER, self).train(False)

    # ------------------------------------------------------------------ host side: sentences -> token ids
    def tokenizer(self):
        """the directory's byte-level BPE through the `tokenizers` package (tokenizer.json, or vocab.json + merges.txt), without its own
        truncation, padding or special tokens: `tokenize` adds those"""
        if self._tokenizer is None:
            self._tokenizer = hfdir.load_tokenizer(      # (TOKENIZERS_PARALLELISM=false as in encoder.py:28)
                self.model_dir, "SBERT_ENCODER", _SBERT_SUBDIRS,
                "SBERT_ENCODER.forward tokenizes with the `tokenizers` package, which is not importable here; "
                "call forward_ids(input_ids, lengths) with ids tokenized elsewhere", bpe_files=True)
        return self._tokenizer

    def tokenize(self, sents):
        """sentences -> (int64 [B, MAX_LENGTH] right-padded with the pad id, int64 [B] lengths): each string stripped, <s> ... </s>
        around it, truncated to MAX_LENGTH tokens INCLUDING the two specials (what SentenceTransformer.tokenize does at
        max_seq_length = TEXT.MAX_LENGTH, encoder.py:37,45)"""
        tok, L = self.tokenizer(), self.max_seq_length
        encs = tok.encode_batch([str(s).strip() for s in sents], add_special_tokens=False)
        ids = torch.full((len(encs), L), self.pad_id, dtype=torch.int64)
        lens = torch.empty(len(encs), dtype=torch.int64)
        for i, e in enumerate(encs):
            row = [self.bos_id] + list(e.ids)[:L - 2] + [self.eos_id]
            ids[i, :len(row)] = torch.tensor(row, dtype=torch.int64)
            lens[i] = len(row)
        return ids, lens

    # ------------------------------------------------------------------ device side
    @torch.no_grad()
    def forward_ids(self, input_ids, lengths):
        """input_ids int64 [B, T] (T <= MAX_LENGTH, right-padded with the pad id), lengths [B] (tokens including <s> and </s>) ->
        words_embs [B, H, MAX_LENGTH], sent_embs [B, H], mask [B, MAX_LENGTH]"""
        w = self._w
        dev = w["word"].device
        input_ids, lengths = torch.as_tensor(input_ids), torch.as_tensor(lengths)
        if input_ids.dim() != 2 or not 1 <= input_ids.size(1) <= self.max_seq_length or lengths.numel() != input_ids.size(0):
            raise ValueError(f"input_ids must be [B, T <= {self.max_seq_length}] with one length per row, got {tuple(input_ids.shape)} / "
                             f"{tuple(lengths.shape)}")
        B, T = input_ids.shape
        if not input_ids.is_cuda:      # host tensors: validate for free
            if int(lengths.min()) < 1 or int(lengths.max()) > T:
                raise ValueError("sentence lengths must lie in [1, T]")
            if int(input_ids.min()) < 0 or int(input_ids.max()) >= self.vocab:
                raise IndexError("token id outside [0, vocab_size)")
        ids = input_ids.to(dev, torch.int64, non_blocking=True).contiguous()
        lens = lengths.to(dev, torch.int32, non_blocking=True).contiguous()
        # GEMM operands in the engine's activation format; the residual stream x, LayerNorm, softmax and the pooling are f32 in every mode
        dt = ops.act_dtype()
        f32 = torch.float32
        x, xh = ops.roberta_embed_ln(ids, lens, w["word"], w["pos"], w["type0"], w["emb_g"], w["emb_b"], self.eps, self.pad_id, out16=dt)
        for i in range(self.nlayers):
            g = lambda n: w[f"{i}.{n}"]
            qkv = ops.linear(x if xh is None else xh, g("wqkv"), g("bqkv"), self.geom_qkv, out_dtype=f32)
            ctx = ops.attention_short(qkv, lens, B, T, self.heads, out_dtype=dt)
            att = ops.linear(ctx, g("wo"), g("bo"), self.geom_o, out_dtype=f32)
            x, xh = ops.add_layernorm(att, x, g("ln1g"), g("ln1b"), self.eps, out16=dt)
            up = ops.linear(x if xh is None else xh, g("w1"), None, self.geom_up, out_dtype=f32)
            act = ops.bias_gelu(up, g("b1"), out_dtype=dt)
            down = ops.linear(act, g("w2"), g("b2"), self.geom_down, out_dtype=f32)
            x, xh = ops.add_layernorm(down, x, g("ln2g"), g("ln2b"), self.eps, out16=dt if i + 1 < self.nlayers else None)
        return ops.sbert_pool(x.view(B, T, self.hidden), lens, self.max_seq_length, self.bert_norm)

    def forward(self, sents, sent_lens=None, **kwargs):
        """sents: a sequence of B strings; sent_lens (word counts upstream, used there only to sort the batch) is not needed"""
        ids, lens = self.tokenize(sents)
        T = int(lens.max())
        return self.forward_ids(ids[:, :T], lens)


class _BasicConv2d(nn.Module):
    """torchvision's BasicConv2d as a parameter container: conv without bias, BatchNorm with eps 1e-3"""

    def __init__(self, cin, cout, k, s, p, eps):
        super(_BasicConv2d, self).__init__()
        self.conv = nn.Conv2d(cin, cout, kernel_size=k, stride=s, padding=p, bias=False)
        self.bn = nn.BatchNorm2d(cout, eps=eps)


class CNN_ENCODER(nn.Module):
    """``CNN_ENCODER(nef)``: AttnGAN's image encoder (model.py CNN_ENCODER).  ``forward(x)``: f32 [B,3,H,W] in [-1, 1] ->
    ``features [B,nef,17,17]`` (``emb_features`` of Mixed_6e's output), ``cnn_code [B,nef]`` (``emb_cnn_code`` of the pooled Mixed_7c
    output), both f32.  ``encode_u8``: the same from uint8 [N,H,W,3].  The 94 BasicConv2d modules and the two projections hold upstream's
    parameters and buffers (no ``fc``, no ``AuxLogits``: AttnGAN's checkpoint has neither); the forward runs on f64-folded f32 copies of
    them through the HIP kernels, in f32 whatever ``ops.set_precision`` says.  Frozen, evaluation mode only.
    ``resize_to``: 299 as upstream; None feeds the images at their own size (at least 75x75; the tests' small maps)."""

    def __init__(self, nef, resize_to=299):
        from xmc_gan_amd import fid as _fid        # (here, not at the top: a run without an image encoder imports no Inception code)
        super(CNN_ENCODER, self).__init__()
        self.nef = int(nef)
        self.resize_to = resize_to
        for name, (cin, cout, k, s, p) in _fid.inception_layers().items():
            parent = self
            *path, leaf = name.split(".")
            for part in path:
                if not hasattr(parent, part):
                    parent.add_module(part, nn.Module())
                parent = getattr(parent, part)
            parent.add_module(leaf, _BasicConv2d(cin, cout, k, s, p, _fid.BN_EPS))
        self.emb_features = nn.Conv2d(768, self.nef, kernel_size=1, stride=1, padding=0, bias=False)      # AttnGAN's conv1x1
        self.emb_cnn_code = nn.Linear(2048, self.nef)
        initrange = 0.1                                                                                   # AttnGAN's init_trainable_weights
        self.emb_features.weight.data.uniform_(-initrange, initrange)
        self.emb_cnn_code.weight.data.uniform_(-initrange, initrange)
        for p_ in self.parameters():
            p_.requires_grad_(False)
        self._folded = None
        super(CNN_ENCODER, self).train(False)

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("CNN_ENCODER runs frozen in eval mode (the DAMSM image encoder is an evaluation network here); "
                                      "training it is not built")
        return super(CNN_ENCODER, self).train(False)

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        """upstream's checkpoints as they are, also with the ``module.`` prefix a DataParallel wrapper leaves on every key"""
        if len(state_dict) and all(k.startswith("module.") for k in state_dict):
            state_dict = {k[len("module."):]: v for k, v in state_dict.items()}
        out = super(CNN_ENCODER, self).load_state_dict(state_dict, strict=strict, **kwargs)
        self._folded = None
        return out

    def _net(self):
        """(the folded trunk, emb_features as (geom, w, None), emb_cnn_code as (geom, w, b)) on the parameters' device; rebuilt when a
        parameter or buffer changes (load_state_dict, .to())"""
        sd = {k: v for k, v in self.state_dict(keep_vars=True).items() if v.is_floating_point()}
        key = tuple((v.data_ptr(), v._version) for v in sd.values())
        if self._folded is None or self._folded[0] != key:
            from xmc_gan_amd import fid as _fid
            dev = self.emb_cnn_code.weight.device
            trunk = _fid.InceptionTrunk(_fid.check_inception_state(sd, "CNN_ENCODER", "the module"), dev, "torchvision")
            frozen = lambda t: nn.Parameter(t.detach().to(dev, torch.float32).contiguous(), requires_grad=False)      # noqa: E731
            cp = ops.pad_to(self.nef, 8)
            bias = torch.zeros(cp, dtype=torch.float32, device=dev)
            bias[:self.nef] = self.emb_cnn_code.bias.detach().float()
            feat = (ops.ConvGeom(768, self.nef, 1, 1, 0), frozen(self.emb_features.weight), None)
            code = (ops.ConvGeom(2048, self.nef, 1, 1, 0), frozen(self.emb_cnn_code.weight), bias)
            self._folded = (key, trunk, feat, code)
        return self._folded[1:]

    def _encode(self, x8):
        trunk, (gf, wf, _), (gc, wc, bc) = self._net()
        mid, pooled = trunk.trunk(x8, with_mixed_6e=True)
        f32 = torch.float32
        feats = ops._conv_fwd_raw(mid, wf, None, gf, _L.ACT_NONE, f32)[..., :self.nef]                        # [B,h,w,nef]
        code = ops._conv_fwd_raw(pooled.view(pooled.shape[0], 1, 1, 2048), wc, bc, gc, _L.ACT_NONE, f32)
        return feats.permute(0, 3, 1, 2).contiguous(), code.view(pooled.shape[0], -1)[:, :self.nef].contiguous()

    def _side(self, hw):
        side = None if self.resize_to is None else (self.resize_to, self.resize_to)
        if min(side or hw) < 75:
            raise ValueError(f"CNN_ENCODER: Inception-v3 needs at least 75x75 pixels, got {tuple(side or hw)}")
        return side

    @torch.no_grad()
    def forward(self, x):
        if self.training:
            raise NotImplementedError("CNN_ENCODER runs frozen in eval mode")
        x = torch.as_tensor(x)
        if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
            raise ValueError(f"CNN_ENCODER: f32 images [B,3,H,W] in [-1, 1] expected, got {x.dtype} {tuple(x.shape)}")
        x = x.detach().to(self.emb_cnn_code.weight.device)
        return self._encode(ops.resize_bilinear_f32(x, self._side(x.shape[2:4])))

    @torch.no_grad()
    def encode_u8(self, u8):
        """uint8 [N,H,W,3] (what `xmc_gan_amd.fid.nchw_to_u8` makes and PIL reads) -> the same pair, from 2 * (b / 255) - 1"""
        u8 = torch.as_tensor(u8)
        if u8.dim() != 4 or u8.shape[-1] != 3 or u8.dtype != torch.uint8:
            raise ValueError(f"CNN_ENCODER: uint8 images [N,H,W,3] expected, got {u8.dtype} {tuple(u8.shape)}")
        u8 = u8.to(self.emb_cnn_code.weight.device)
        return self._encode(ops.fid_resize_u8(u8, self._side(u8.shape[1:3])))
