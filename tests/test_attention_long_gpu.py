"""`ops.attention_long` (csrc/attention_long.hip) on the GPU: f32 MFMA attention for 1 <= T <= 1024 with key padding and the causal mask,
against tests/clip_ref.py's `attention` in f64 on the CPU; the properties its tiling must not break (a sample's bytes depend neither on T
nor on the batch nor on what lies behind its length; causal == key padding with growing lengths, bit for bit); the refusals.

Error figure: e = max |got - want| / rms(want).  The bar of every comparison is computed by the test: 4 x e_f32, the same figure of the same
restatement evaluated in f32 by torch on the CPU on the same inputs (the tiled softmax rescales its accumulator once per key tile and sums in
another order: a handful of f32 roundings beyond the plain evaluation).  Measured on the MI355X: the figures each test prints, DESIGN.md 7q."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ref as R
import xmc_gan_amd.lib as L
from xmc_gan_amd import ops

DEV = torch.device("cuda", 0)
B, HEADS = 3, 2
H = HEADS * 64
FACTOR = 4.0


def _rn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _err(got, want):
    want = torch.as_tensor(want).double()
    return float((got.detach().double().cpu() - want).abs().max() / want.pow(2).mean().sqrt())


def _reference(qkv, T, lens, causal, dtype):
    """the restatement per sample on its first len rows (rows behind it: zeros), computed in `dtype`; [B*T, H] in that dtype"""
    nb = qkv.shape[0] // T
    x = qkv.view(nb, T, 3 * H).to(dtype)
    out = torch.zeros(nb, T, H, dtype=dtype)
    for b in range(nb):
        n = T if lens is None else int(lens[b])
        if n:
            q, k, v = (t.contiguous() for t in x[b:b + 1, :n].split(H, dim=2))
            out[b, :n] = R.attention(q, k, v, HEADS, causal)[0]
    return out.view(nb * T, H)


_refs = {}


def _case(T, lens, causal, seed):
    """(qkv on the CPU, want f64, bar): computed once per case and shared"""
    key = (T, None if lens is None else tuple(lens), causal, seed)
    if key not in _refs:
        qkv = _rn(B * T, 3 * H, seed=seed)
        want = _reference(qkv, T, lens, causal, torch.float64)
        e32 = _err(_reference(qkv, T, lens, causal, torch.float32), want)
        _refs[key] = qkv, want, FACTOR * e32
    return _refs[key]


def _run(qkv, T, lens, causal, nb=B):
    ld = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    return ops.attention_long(qkv.to(DEV), ld, nb, T, HEADS, causal=causal)


def _check(name, T, lens, causal, seed):
    qkv, want, bar = _case(T, lens, causal, seed)
    got = _run(qkv, T, lens, causal)
    e = _err(got, want)
    print(f"attention_long {name} T {T} lens {lens}: e {e:.3e}, e_f32 {bar / FACTOR:.3e}, bar {bar:.3e}")
    assert got.dtype == torch.float32 and tuple(got.shape) == (B * T, H) and bool(torch.isfinite(got).all())
    assert e <= bar
    return qkv, got


@pytest.mark.parametrize("T", [1, 33, 64, 65, 77, 129, 197, 257])
def test_full_length(T):
    """one row, a partial MFMA tile, exactly one key tile, one key over, two tiles plus one, ViT-B/16's and L/14's token counts"""
    _check("non-causal", T, None, False, seed=100 + T)


@pytest.mark.parametrize("lens", [[129, 65, 1], [0, 64, 128]], ids=["129-65-1", "0-64-128"])
def test_ragged_lengths(lens):
    T = 129
    qkv, got = _check("ragged", T, lens, False, seed=7)
    got = got.view(B, T, H)
    for b, n in enumerate(lens):
        assert bool((got[b, n:] == 0).all())                          # rows >= len: zeros (a length-0 sample: all of them)
    # what lies behind a sample's length is never read: NaN there, equal bytes
    poisoned = qkv.clone().view(B, T, 3 * H)
    for b, n in enumerate(lens):
        poisoned[b, n:] = float("nan")
    again = _run(poisoned.view(B * T, 3 * H), T, lens, False)
    assert torch.equal(again.view(B, T, H), got)


@pytest.mark.parametrize("T", [7, 64, 65, 77, 257])
def test_causal(T):
    qkv, got = _check("causal", T, None, True, seed=200 + T)
    assert torch.equal(got.view(B, T, H)[:, 0].cpu(), qkv.view(B, T, 3 * H)[:, 0, 2 * H:])        # query 0 sees key 0 alone: v[0]


def test_causal_with_lengths():
    T, lens = 77, [77, 40, 1]
    _, got = _check("causal + lens", T, lens, True, seed=9)
    for b, n in enumerate(lens):
        assert bool((got.view(B, T, H)[b, n:] == 0).all())


def test_causal_is_key_padding_with_growing_lengths():
    """one sample T times with the lengths 1 .. T: query b of the sample that is b + 1 tokens long sees the keys 0 .. b, as causal query b
    does -- the property test_clip_gpu.py holds the short kernels to, here across a key-tile boundary"""
    T = 77
    qkv = _rn(T, 3 * H, seed=41).to(DEV)
    lens = torch.arange(1, T + 1, dtype=torch.int32, device=DEV)
    padded = ops.attention_long(qkv.repeat(T, 1), lens, T, T, HEADS).view(T, T, H)
    causal = ops.attention_long(qkv, None, 1, T, HEADS, causal=True)
    assert torch.equal(padded[torch.arange(T), torch.arange(T)], causal)


def test_bytes_depend_on_the_sample_alone():
    T = 129
    qkv, _, _ = _case(T, None, False, 100 + T)
    whole = _run(qkv, T, None, False).view(B, T, H)
    assert torch.equal(_run(qkv, T, None, False).view(B, T, H), whole)                                 # two runs
    alone = _run(qkv.view(B, T, 3 * H)[1].contiguous(), T, None, False, nb=1)
    assert torch.equal(alone.view(T, H), whole[1])                                                     # the batch and the place in it
    # the padding: a sample of 65 tokens in rows of 129 and in rows of 65
    lens = [129, 65, 1]
    ragged = _run(qkv, T, lens, False).view(B, T, H)
    tight = _run(qkv.view(B, T, 3 * H)[1, :65].contiguous(), 65, None, False, nb=1)
    assert torch.equal(tight.view(65, H), ragged[1, :65])
    # causal: 70 rows alone and the first 70 of 77 rows, noise in the other 7
    x = _rn(B, 77, 3 * H, seed=3)
    long_ = _run(x.reshape(B * 77, 3 * H), 77, None, True).view(B, 77, H)
    short = _run(x[:, :70].reshape(B * 70, 3 * H), 70, None, True).view(B, 70, H)
    assert torch.equal(long_[:, :70], short)


@pytest.mark.parametrize("T", [7, 64])
def test_against_the_short_kernels(T):
    """the same function as `attention_short` / `attention_causal` where both run: each within its bar of the f64 restatement (not bitwise:
    another summation order)"""
    for causal in (False, True):
        qkv, want, bar = _case(T, None, causal, 300 + T)
        dq = qkv.to(DEV)
        long_ = ops.attention_long(dq, None, B, T, HEADS, causal=causal)
        short = ops.attention_causal(dq, B, T, HEADS) if causal else \
            ops.attention_short(dq, torch.full((B,), T, dtype=torch.int32, device=DEV), B, T, HEADS)
        el, es = _err(long_, want), _err(short, want)
        between = float((long_ - short).abs().max()) / float(want.pow(2).mean().sqrt())
        print(f"attention_long / short T {T} causal {causal}: long {el:.3e}, short {es:.3e}, between {between:.3e}, bar {bar:.3e}")
        assert el <= bar and between <= 2 * bar                # (the short kernels' own bars: tests/test_clip_gpu.py, test_sbert_gpu.py)


def test_refusals():
    with pytest.raises(AssertionError):
        ops.attention_long(torch.zeros(0, 3 * 64, device=DEV), None, 1, 0, 1)
    with pytest.raises(AssertionError):
        ops.attention_long(torch.zeros(1025, 3 * 64, device=DEV), None, 1, 1025, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.attention_long(torch.zeros(4, 3 * 64), None, 1, 4, 1)
    x, y = torch.zeros(4, 3 * 32, device=DEV), torch.zeros(4, 32, device=DEV)
    with pytest.raises(L.XmcHipError, match="XMC_ESHAPE"):
        L.call("xmc_attention_long", x.data_ptr(), None, y.data_ptr(), 1, 4, 1, 32, 0, None)
    assert ops.ATTENTION_LONG_MAX_T == 1024 and ops.ATTENTION_MAX_T == 64
