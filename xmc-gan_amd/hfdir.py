"""Reading a Hugging Face model directory without third-party model code: what `SBERT_ENCODER` (xmc_gan/model/encoder.py) and `CLIPScorer`
(clip.py) share.  ``who`` is the class name the messages start with; ``subdirs`` are the places a file is looked for, relative to the
directory and in that order ("": the directory itself)."""
import os

import torch
import torch.nn as nn


def find(model_dir, names, subdirs=("",)):
    """the first of ``names`` that is a file, or None"""
    for sub in subdirs:
        for n in names:
            p = os.path.join(model_dir, sub, n)
            if os.path.isfile(p):
                return p
    return None


def read_weights(model_dir, who, subdirs=("",), where=""):
    """the state dict: model.safetensors when the `safetensors` package imports, else pytorch_model.bin.  ``where`` ends the message of a
    directory that holds neither (the places that were searched)"""
    st = find(model_dir, ("model.safetensors",), subdirs)
    if st is not None:
        try:
            from safetensors.torch import load_file
            return load_file(st)
        except ImportError:
            pass
    pt = find(model_dir, ("pytorch_model.bin",), subdirs)
    if pt is None:
        what = "pytorch_model.bin (model.safetensors is there, but the safetensors package is not importable)" if st \
            else "model.safetensors / pytorch_model.bin"
        raise ImportError(f"{who}: {model_dir} holds no {what}{where}")
    return torch.load(pt, map_location="cpu", weights_only=True)


def weight_access(sd, who, model_dir, cj, device=None):
    """(take, frozen): ``take(key, shape)`` is the f32 tensor of ``sd`` under ``key``, checked against the shape that the config file
    ``cj`` implies; ``frozen(t)`` makes a contiguous Parameter without a gradient of it (on ``device``, when one is named), so that
    the packed copies of a GEMM weight are cached until it changes"""
    def take(key, shape):
        if key not in sd:
            raise ImportError(f"{who}: the weights in {model_dir} lack {key!r}")
        t = sd[key].detach().float()
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{who}: {key} is {tuple(t.shape)}, {cj} says {tuple(shape)}")
        return t

    def frozen(t):
        return nn.Parameter((t if device is None else t.to(device)).contiguous(), requires_grad=False)

    return take, frozen


def load_tokenizer(model_dir, who, subdirs, hint, bpe_files=False):
    """the directory's tokenizer.json through the `tokenizers` package (``hint``: the ImportError's text when that is not importable), or,
    with ``bpe_files``, a byte-level BPE without prefix space (RoBERTa's) from vocab.json + merges.txt; without truncation and padding of
    its own"""
    try:
        import tokenizers
    except ImportError as e:
        raise ImportError(hint) from e
    os.environ.setdefault("TOKENIZERS_PARALLELISM", "false")
    tj = find(model_dir, ("tokenizer.json",), subdirs)
    if tj is not None:
        tok = tokenizers.Tokenizer.from_file(tj)
    elif not bpe_files:
        raise ImportError(f"{who}: {model_dir} holds no tokenizer.json")
    else:
        vj, mt = find(model_dir, ("vocab.json",), subdirs), find(model_dir, ("merges.txt",), subdirs)
        if vj is None or mt is None:
            raise ImportError(f"{who}: {model_dir} holds neither tokenizer.json nor vocab.json + merges.txt")
        tok = tokenizers.Tokenizer(tokenizers.models.BPE.from_file(vj, mt))
        tok.pre_tokenizer = tokenizers.pre_tokenizers.ByteLevel(add_prefix_space=False)
    tok.no_truncation()
    tok.no_padding()
    return tok
