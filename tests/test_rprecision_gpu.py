"""R-precision on the GPU (xmc_gan_amd/rprecision.py, xmc_gan/model/encoder.py CNN_ENCODER, csrc/retrieval.hip and the additions to
csrc/fid.hip) against the plain-torch f64 restatement in tests/damsm_ref.py and torch's own CPU f64 functions.

The conventions are tests/test_fid_gpu.py's: the error figure is max |got - want| over the rms of `want`, every bar is 1.5 x the figure
measured on the MI355X, which is written beside it, and a figure above 1e-4 would be a bug to find, not a bar to set."""
import json
import logging
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import damsm_ref
import fid_ref
import xmc_ref as X
from xmc_gan.model.encoder import CNN_ENCODER, RNN_ENCODER
from xmc_gan_amd import fid as FID
from xmc_gan_amd import lib as L
from xmc_gan_amd import ops
from xmc_gan_amd import rprecision as RP

DEV = torch.device("cuda", 0)
NEF = 32


def _err(got, want):
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double()
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((got - want).abs().max() / want.pow(2).mean().sqrt())


def _nhwc(x_nchw):
    return x_nchw.permute(0, 2, 3, 1).float().contiguous().to(DEV)


def _nchw(y_nhwc, c=None):
    y = y_nhwc.cpu().permute(0, 3, 1, 2)
    return y if c is None else y[:, :c]


@pytest.fixture(scope="module")
def net():
    """(the restatement, CNN_ENCODER(32) without a resize on the device) from one random state dict"""
    sd = damsm_ref.random_state_dict(7, NEF)
    enc = CNN_ENCODER(NEF, resize_to=None)
    enc.load_state_dict(sd, strict=True)
    return damsm_ref.Reference(sd), enc.to(DEV).eval()


@pytest.fixture(scope="module")
def damsm256(tmp_path_factory):
    """(the restatement, the weights file) of a random 256-wide encoder: the width of the RNN presets' sentence codes"""
    sd = damsm_ref.random_state_dict(11, 256)
    path = str(tmp_path_factory.mktemp("damsm") / "image_encoder_random.pth")
    torch.save(sd, path)
    return damsm_ref.Reference(sd), path


# ------------------------------------------------------------------------------------------ the count_include_pad=True pool
# measured, by (map, channels); 1x1 maps: one pixel / 9
POOL_PAD_MEASURED = {(7, 7, 8): 5.356e-07, (7, 7, 288): 5.932e-07, (6, 6, 8): 2.845e-07, (6, 6, 288): 5.276e-07,
                     (3, 5, 8): 2.783e-07, (3, 5, 288): 4.590e-07, (1, 1, 8): 3.514e-08, (1, 1, 288): 1.220e-07}


@pytest.mark.parametrize("c", [8, 288])
@pytest.mark.parametrize("h,w", [(7, 7), (6, 6), (3, 5), (1, 1)])
def test_pool3x3_avg_pad(h, w, c):
    x = torch.randn(3, c, h, w, generator=torch.Generator().manual_seed(h * 10 + w)).double()
    xd = _nhwc(x)
    want = F.avg_pool2d(x, 3, 1, 1, count_include_pad=True)
    e = _err(_nchw(ops.pool3x3(xd, "avg_pad", 1)), want)
    print(f"pool avg_pad {h}x{w} C{c}: {e:.3e}")
    assert e <= 1.5 * POOL_PAD_MEASURED[(h, w, c)]
    # a map of ones: the window holds 4 in-image pixels at a corner, 6 at an edge, 9 inside
    ones = ops.pool3x3(torch.ones_like(xd), "avg_pad", 1).cpu()
    inside = lambda n, i: 3 - (i == 0) - (i == n - 1) if n > 1 else 1      # noqa: E731
    want1 = torch.tensor([[inside(h, i) * inside(w, j) for j in range(w)] for i in range(h)], dtype=torch.float32) / 9.0
    assert torch.equal(ones, want1[None, :, :, None].expand_as(ones))
    if h >= 3 and w >= 3:
        assert float(ones[0, 0, 0, 0]) == np.float32(4) / np.float32(9) and float(ones[0, 0, 1, 0]) == np.float32(6) / np.float32(9)
        assert float(ones[0, 1, 1, 0]) == 1.0


def test_pool3x3_avg_pad_refuses_stride_2():
    x = torch.zeros((1, 5, 5, 8), dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError):
        ops.pool3x3(x, "avg_pad", 2)
    p = ops._p(x)
    assert L.load().xmc_pool3x3(p, p, 1, 5, 5, 8, L.POOL_AVG_PAD, 2, None) == -1          # XMC_EINVAL, nothing launched


# ------------------------------------------------------------------------------------------ float front end
@pytest.mark.parametrize("h,w,measured", [(64, 64, 3.729e-07), (256, 256, 3.978e-07), (300, 400, 3.944e-07)])
def test_resize_f32(h, w, measured):
    x = torch.rand(3, 3, h, w, generator=torch.Generator().manual_seed(h)) * 2 - 1
    got = ops.resize_bilinear_f32(x.to(DEV), (299, 299))
    assert tuple(got.shape) == (3, 299, 299, 8) and got.dtype == torch.float32
    assert not got[..., 3:].any()
    e = _err(_nchw(got, 3), F.interpolate(x.double(), size=(299, 299), mode="bilinear", align_corners=False))
    print(f"resize f32 {h}x{w} -> 299: {e:.3e}")
    assert e <= 1.5 * measured


def test_resize_f32_same_size_is_exact():
    g = torch.Generator().manual_seed(2)
    for shape in ((3, 3, 299, 299), (2, 3, 5, 7)):
        x = torch.randn(shape, generator=g)
        for out_hw in (None, shape[2:]):
            got = ops.resize_bilinear_f32(x.to(DEV), out_hw).cpu()
            assert torch.equal(got[..., :3], x.permute(0, 2, 3, 1)) and not got[..., 3:].any()
    with pytest.raises(ValueError):
        ops.resize_bilinear_f32(torch.zeros((1, 4, 4, 4), device=DEV))
    with pytest.raises(ValueError):
        ops.resize_bilinear_f32(torch.zeros((1, 3, 4, 4), device=DEV, dtype=torch.float64))


@pytest.mark.parametrize("h,w,measured", [(64, 64, 1.246e-06), (300, 400, 1.259e-06)])
def test_resize_f32_agrees_with_resize_u8(h, w, measured):
    """the two front ends on the same picture: bytes b on one side, the floats 2 (b / 255) - 1 on the other.  They blend in a different
    order (the byte path scales after the blend), so they agree to rounding, not to the bit."""
    u8 = torch.randint(0, 256, (3, h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(w))
    x = (2.0 * (u8.float() / 255.0) - 1.0).permute(0, 3, 1, 2).contiguous()
    a, b = ops.resize_bilinear_f32(x.to(DEV), (299, 299)), ops.fid_resize_u8(u8.to(DEV), (299, 299))
    e = _err(a, b.double().cpu())
    print(f"resize f32 vs u8 {h}x{w} -> 299: {e:.3e}")
    assert e <= 1.5 * measured


# ------------------------------------------------------------------------------------------ blocks and the whole encoder
@pytest.mark.parametrize("name,hw,measured", [("Mixed_5b", 5, 3.259e-06), ("Mixed_6b", 5, 6.419e-06), ("Mixed_7b", 5, 6.875e-06),
                                              ("Mixed_7c", 5, 8.387e-06)])
def test_torchvision_block(net, name, hw, measured):
    ref, enc = net
    x = torch.randn(2, FID.BLOCK_IN[name], hw, hw, generator=torch.Generator().manual_seed(hw)).abs().double()
    want = ref.block(name, x)
    trunk = enc._net()[0]
    assert trunk.variant == "torchvision"
    e = _err(_nchw(trunk.block(name, _nhwc(x))), want)
    print(f"torchvision {name} on {hw}x{hw}: {e:.3e}")
    assert e <= 1.5 * measured
    # and the pool branch is what separates the variants: the FID restatement of the same weights differs visibly
    assert _err(want, fid_ref.Reference(ref.sd).block(name, x)) > 1e-3


def test_encoder_without_resize(net):
    ref, enc = net
    u8 = damsm_ref.structured_images(3, 75, 75)
    x = (2.0 * (u8.float() / 255.0) - 1.0).permute(0, 3, 1, 2).contiguous()
    want_f, want_c = ref.forward(x, None)
    got_f, got_c = enc(x.to(DEV))
    assert tuple(got_f.shape) == (3, NEF, 3, 3) and tuple(got_c.shape) == (3, NEF) and got_f.dtype == got_c.dtype == torch.float32
    ef, ec = _err(got_f, want_f), _err(got_c, want_c)
    spread = float((want_c - want_c.mean(0)).pow(2).mean().sqrt() / want_c.pow(2).mean().sqrt())
    print(f"encoder 75x75 N3: features {ef:.3e}, code {ec:.3e} (code rms {float(want_c.pow(2).mean().sqrt()):.3f}, spread between images {spread:.3f})")
    assert ef <= 1.5 * 3.059e-06                # measured: 3.059e-06
    assert ec <= 1.5 * 2.812e-06                # measured: 2.812e-06 (code rms 0.767, spread between the three images 0.053 of it)
    with pytest.raises(ValueError):
        enc(x[:, :, :70].to(DEV))
    with pytest.raises(ValueError):
        enc(x.double().to(DEV))
    with pytest.raises(NotImplementedError):
        enc.train()
    assert not enc.training


def test_encoder_with_resize(net):
    ref, enc = net
    import copy
    enc299 = copy.copy(enc)
    enc299.resize_to = 299
    u8 = damsm_ref.structured_images(2, 64, 64)
    x = (2.0 * (u8.float() / 255.0) - 1.0).permute(0, 3, 1, 2).contiguous()
    want_f, want_c = ref.forward(x, 299)
    got_f, got_c = enc299(x.to(DEV))
    assert tuple(got_f.shape) == (2, NEF, 17, 17) and tuple(got_c.shape) == (2, NEF)
    ef, ec = _err(got_f, want_f), _err(got_c, want_c)
    print(f"encoder 64x64 -> 299 N2: features {ef:.3e}, code {ec:.3e}")
    assert ef <= 1.5 * 6.612e-06                # measured: 6.612e-06
    assert ec <= 1.5 * 2.443e-06                # measured: 2.443e-06


def test_two_paths_one_network(net):
    _, enc = net
    u8 = damsm_ref.structured_images(2, 75, 3)
    x = (2.0 * (u8.float() / 255.0) - 1.0).permute(0, 3, 1, 2).contiguous()
    (f_a, c_a), (f_b, c_b) = enc(x.to(DEV)), enc.encode_u8(u8.to(DEV))
    assert torch.equal(f_a, f_b) and torch.equal(c_a, c_b)
    with pytest.raises(ValueError):
        enc.encode_u8(x.to(DEV))


def test_encoder_ignores_the_precision_mode(net):
    _, enc = net
    u8 = damsm_ref.structured_images(2, 75, 4)
    try:
        a = enc.encode_u8(u8)
        ops.set_precision("f16")
        b = enc.encode_u8(u8)
        ops.set_precision("fp32")
        c = enc.encode_u8(u8)
    finally:
        ops.set_precision("bf16")
    for i in range(2):
        assert torch.equal(a[i], b[i]) and torch.equal(a[i], c[i])


def test_folded_copies_follow_the_parameters(net):
    _, enc = net
    import copy
    u8 = damsm_ref.structured_images(1, 75, 5)
    other = copy.deepcopy(enc)
    before = other.encode_u8(u8)[1]
    sd = damsm_ref.random_state_dict(8, NEF)
    other.load_state_dict({"module." + k: v for k, v in sd.items()}, strict=True)          # (and the DataParallel prefix)
    after = other.encode_u8(u8)[1]
    assert not torch.equal(before, after)
    want = damsm_ref.Reference(sd).forward_u8(u8, None)[1]
    e = _err(after, want)
    print(f"encoder after load_state_dict: code {e:.3e}")
    assert e <= 1.5 * 2.189e-06                    # measured: 2.189e-06


# ------------------------------------------------------------------------------------------ the retrieval kernel
# (N, M, K, D) -> (seed, the f64 reference's smallest |score[n][k] - score[n][0]| over k >= 1 at that seed); the seeds were chosen on the CPU
# (the first from 0 whose margin is at least 1e-5: 100 x the f32 rounding of a cosine) -- see _retrieval_case
RETRIEVAL_CASES = {(1, 1, 1, 8): (0, None), (5, 7, 2, 256): (0, 3.834370e-02), (67, 40, 100, 256): (0, 3.389640e-05), (3, 9, 4, 1024): (0, 5.791252e-03)}
RETRIEVAL_MEASURED = {(1, 1, 1, 8): 1.525e-07, (5, 7, 2, 256): 1.761e-07, (67, 40, 100, 256): 5.676e-07, (3, 9, 4, 1024): 3.332e-07}


def _retrieval_case(N, M, K, D, seed):
    """random codes and a candidate table whose other columns never name the own caption's row (K may exceed M: rows repeat)"""
    g = torch.Generator().manual_seed(seed)
    img, txt = torch.randn(N, D, generator=g), torch.randn(M, D, generator=g)
    own = torch.randint(0, M, (N,), generator=g)
    cand = torch.empty((N, K), dtype=torch.int32)
    cand[:, 0] = own
    if K > 1:
        other = torch.randint(0, M - 1, (N, K - 1), generator=g)
        cand[:, 1:] = (other + (other >= own[:, None]).long()).int()
    return img, txt, cand


def _margin(score):
    return float((score[:, 1:] - score[:, :1]).abs().min()) if score.shape[1] > 1 else None


@pytest.mark.parametrize("shape", list(RETRIEVAL_CASES))
def test_rprecision_kernel(shape):
    seed, margin = RETRIEVAL_CASES[shape]
    N, M, K, D = shape
    img, txt, cand = _retrieval_case(N, M, K, D, seed)
    want_s, want_r = damsm_ref.cosine_scores(img, txt, cand)
    if K > 1:
        assert _margin(want_s) >= 1e-5 and abs(_margin(want_s) - margin) <= 1e-3 * margin
    rank, score = ops.rprecision(img.to(DEV), txt.to(DEV), cand.to(DEV), return_scores=True)
    assert rank.dtype == torch.int32 and tuple(rank.shape) == (N,) and tuple(score.shape) == (N, K) and score.dtype == torch.float32
    e = _err(score, want_s)
    print(f"rprecision N{N} M{M} K{K} D{D}: scores {e:.3e}, margin {margin}, kernel {L.load().xmc_last_kernel().decode()}")
    assert e <= 1.5 * RETRIEVAL_MEASURED[shape]
    assert torch.equal(rank.cpu().long(), want_r)                           # every row
    # the same bytes again, with and without the score output, and from a host table
    rank2, score2 = ops.rprecision(img.to(DEV), txt.to(DEV), cand.to(DEV), return_scores=True)
    assert torch.equal(rank, rank2) and torch.equal(score.view(torch.int32), score2.view(torch.int32))
    assert torch.equal(ops.rprecision(img.to(DEV), txt.to(DEV), cand), rank)


def test_rprecision_planted_cases():
    N, M, K, D = 5, 9, 4, 256
    g = torch.Generator().manual_seed(1)
    img, txt = torch.randn(N, D, generator=g), torch.randn(M, D, generator=g)
    cand = torch.tensor([[0, 3, 0, 5],                 # the own caption again: an exact tie, not counted
                         [1, 2, 4, 6],                 # a planted winner at column 1
                         [7, 3, 5, 6],                 # an all-zero image row: every score 0 through the clamp
                         [M - 1, 0, 3, M - 1],         # the last row of txt is a valid candidate
                         [5, 0, 3, 6]], dtype=torch.int32)      # a NaN image row: the own caption scores NaN
    txt[0] = img[0] + 0.1 * txt[0]                     # row 0's caption matches: only the tie could beat it
    txt[1], txt[2] = img[1] + 0.3 * txt[1], 3.0 * img[1]
    img[2] = 0.0
    img[4, 7] = float("nan")
    want_s, want_r = damsm_ref.cosine_scores(img, txt, cand)
    assert want_r.tolist() == [0, 1, 0, int(want_r[3]), K]
    rank, score = ops.rprecision(img.to(DEV), txt.to(DEV), cand.to(DEV), return_scores=True)
    rank, score = rank.cpu(), score.cpu()
    assert rank.tolist() == want_r.tolist()
    assert score[0, 2] == score[0, 0] and float(score[1, 1]) > float(score[1, 0]) > 0.9
    assert torch.equal(score[2], torch.zeros(K)) and torch.isnan(score[4]).all()
    e = _err(score[:4], want_s[:4])
    print(f"rprecision planted cases: scores {e:.3e}")
    assert e <= 1.5 * 2.411e-07                    # measured: 2.411e-07


def test_rprecision_wrapper_refuses_what_the_kernel_cannot_take():
    z = lambda *s: torch.zeros(s, device=DEV)      # noqa: E731
    cand = torch.zeros((2, 3), dtype=torch.int32)
    for bad in (lambda: ops.rprecision(z(2, 6), z(4, 6), cand),                               # D % 4
                lambda: ops.rprecision(z(2, 1028), z(4, 1028), cand),                         # D > 1024
                lambda: ops.rprecision(z(2, 8), z(4, 8), cand + 4),                           # an index past the last row
                lambda: ops.rprecision(z(2, 8), z(4, 8), cand - 1),
                lambda: ops.rprecision(z(2, 8), z(4, 8), cand.long()),
                lambda: ops.rprecision(z(2, 8).double(), z(4, 8), cand),                      # not f32
                lambda: ops.rprecision(z(2, 8), z(4, 8).bfloat16(), cand),
                lambda: ops.rprecision(z(2, 8), z(4, 12), cand),
                lambda: ops.rprecision(z(3, 8), z(4, 8), cand)):
        with pytest.raises(ValueError):
            bad()
    assert ops.rprecision(z(2, 8), z(4, 8), cand + 3).tolist() == [0, 0]                      # M - 1 is accepted


# ------------------------------------------------------------------------------------------ end to end
E2E_SEED, E2E_MARGIN = 1, 2.016118e-03      # chosen on the CPU: the first seed from 0 whose f64 margin is at least 1e-3 (100 x the encoder's error)


def _mini_cfg(tmp_path):
    from test_sample_gpu import _use_cfg, _yml
    return _use_cfg(_yml(tmp_path))


def _e2e_inputs(cfg, seed, n=16):
    """(uint8 images [n,75,75,3], token ids, lengths, the RNN encoder's random parameters)"""
    shapes = X.rnn_encoder_shapes(cfg.TEXT.VOCA_SIZE, cfg.TEXT.EMBEDDING_DIM)
    caps, lens = X.synth_captions(n, cfg.TEXT.MAX_LENGTH, cfg.TEXT.VOCA_SIZE, seed=seed)
    return damsm_ref.structured_images(n, 75, seed), caps, lens, X.synth_rnn_params(shapes, seed)


def _e2e_reference(ref, cfg, u8, caps, lens, P, k, seed):
    """(f64 scores, f64 ranks, the table) of the restatement: image codes without a resize, the oracle's RNN encoder in f64"""
    codes = ref.forward_u8(u8, None)[1]
    sent = X.rnn_encoder({key: v.double() for key, v in P.items()}, caps, lens, cfg.TEXT.MAX_LENGTH)[1]
    table = RP.candidate_table(np.arange(len(u8)), np.arange(len(u8)), k, seed)
    score, rank = damsm_ref.cosine_scores(codes, sent, torch.from_numpy(table))
    return score, rank, table


def test_rprecision_end_to_end(damsm256, tmp_path):
    from xmc_gan.config import gan
    ref, path = damsm256
    try:
        cfg = _mini_cfg(tmp_path)
        u8, caps, lens, P = _e2e_inputs(cfg, E2E_SEED)
        score, rank, table = _e2e_reference(ref, cfg, u8, caps, lens, P, 8, E2E_SEED)
        margin = _margin(score)
        print(f"end to end: f64 margin {margin:.3e}, hits {(rank == 0).long().tolist()}")
        assert margin >= 1e-3 and abs(margin - E2E_MARGIN) <= 1e-3 * E2E_MARGIN
        text = RNN_ENCODER(cfg)
        text.load_state_dict(P, strict=True)
        text = text.to(DEV).eval()
        image = RP.load_image_encoder(path, None, DEV)
        image.resize_to = None
        assert image.nef == 256 and RP.usable_with(text, image) is None
        rp = RP.RPrecision(k=8, splits=4, seed=E2E_SEED)
        for lo, hi in ((0, 5), (5, 16)):
            rp.update(image.encode_u8(u8[lo:hi])[1], text(caps[lo:hi], lens[lo:hi])[1])
        hits, used = rp.hits()
        assert np.array_equal(used, table) and hits.tolist() == (rank == 0).long().tolist()
        out = rp.finalize()
        want = np.array([100.0 * hits[i * 4:(i + 1) * 4].mean() for i in range(4)])
        assert out["n"] == 16 and out["k"] == 8 and out["splits"] == 4 and out["per_split"] == want.tolist()
        assert out["r_precision"] == want.mean() and out["std"] == want.std()
    finally:
        gan.reset_cfg()
        ops.set_precision("bf16")


# ------------------------------------------------------------------------------------------ where it surfaces
def _logger(name):
    lines = []
    logger = logging.getLogger(name)
    logger.setLevel(logging.INFO)
    handler = logging.Handler()
    handler.emit = lambda rec: lines.append(rec.getMessage())
    logger.handlers[:] = [handler]
    return logger, lines


def test_eval_reports_rprecision(damsm256, tmp_path):
    import xmc_gan.train_gan as tg
    from xmc_gan.config import gan
    _, weights = damsm256
    try:
        cfg = _mini_cfg(tmp_path)
        torch.manual_seed(2)
        netG, _, _, _ = tg.build_models(DEV)
        text = RNN_ENCODER(cfg).to(DEV).eval()
        # 13 distinct batches of 8: k = 100 needs 99 captions of other images
        loader = tg.SyntheticCOCO(13, 8, cfg.IMG.SIZE, cfg.TEXT.MAX_LENGTH, 1, cfg.TEXT.VOCA_SIZE, distinct=13)
        logger, lines = _logger("rprecision-eval-test")
        rows = []
        writer = type("W", (), {"add_scalar": lambda self, tag, v, step: rows.append((tag, v, step))})()
        kw = dict(loader=loader, state_epoch=7, text_encoder=text, netG=netG, logger=logger, num_samples=104, writer=writer)
        metrics = {}
        out = tg.eval(damsm_image_encoder=weights, metrics=metrics, **kw)
        assert isinstance(out, tuple) and len(out) == 2 and out[1] is None                 # (images, FID): unchanged, and no FID was asked for
        assert tuple(out[0].shape) == (104, 3, cfg.IMG.SIZE, cfg.IMG.SIZE) and out[0].dtype == torch.uint8
        r = metrics["r_precision"]
        assert set(metrics) == {"r_precision", "std", "n", "k", "splits", "per_split"} and (metrics["n"], metrics["k"], metrics["splits"]) == (104, 100, 10)
        assert 0.0 <= r <= 100.0 and len(metrics["per_split"]) == 10 and r == np.mean(metrics["per_split"])
        assert lines[-1] == f" epoch 7, R-precision : {r} +- {metrics['std']} (k=100, n=104)"
        assert rows == [("R_precision", r, 7)]
        # without the weights: the lines and scalars of before
        del lines[:], rows[:]
        os.environ.pop("XMC_DAMSM_IMAGE_ENCODER", None)
        out = tg.eval(**kw)
        assert not any("R-precision" in line for line in lines) and not any(tag == "R_precision" for tag, _, _ in rows)
        # a sentence encoder that is not the DAMSM caption encoder: one line says so
        del lines[:]
        sbert_like = tg.SyntheticTextEncoder(cfg.TEXT.EMBEDDING_DIM, cfg.TEXT.MAX_LENGTH, 1, DEV)
        metrics = {}
        tg.eval(damsm_image_encoder=weights, metrics=metrics, **dict(kw, text_encoder=sbert_like))
        told = [line for line in lines if "R-precision" in line]
        assert len(told) == 1 and "not computed" in told[0] and "SyntheticTextEncoder" in told[0] and metrics == {} and rows == []
    finally:
        gan.reset_cfg()
        ops.set_precision("bf16")


def test_cli_and_sample_agree(damsm256, tmp_path, capsys):
    import xmc_gan.rprecision as cli
    import xmc_gan.sample as sample
    import xmc_gan.train_gan as tg
    from test_sample_gpu import _use_cfg, _yml
    from xmc_gan.config import gan
    _, weights = damsm256
    try:
        yml = _yml(tmp_path)
        cfg = _use_cfg(yml)
        torch.manual_seed(4)
        torch.save(tg.build_models(DEV)[0].state_dict(), tmp_path / "netG.pth")
        torch.save(RNN_ENCODER(cfg).state_dict(), tmp_path / "text.pth")
        ids, lens = X.synth_captions(6, cfg.TEXT.MAX_LENGTH, cfg.TEXT.VOCA_SIZE, seed=9)
        np.save(tmp_path / "ids.npy", ids.numpy())
        gan.reset_cfg()
        base = ["--cfg", yml, "--checkpoint", str(tmp_path / "netG.pth"), "--out", str(tmp_path / "out"), "--token_ids", str(tmp_path / "ids.npy"),
                "--text_encoder", str(tmp_path / "text.pth"), "--n_per_caption", "2", "--grid_max", "0", "--seed", "3"]
        with pytest.raises(SystemExit, match="damsm_image_encoder"):
            sample.main(base + ["--rprecision", "--damsm_image_encoder", str(tmp_path / "nope.pth")])
        gan.reset_cfg()
        man = sample.main(base + ["--rprecision", "--damsm_image_encoder", weights, "--rp_k", "4", "--rp_splits", "3"])
        r = man["r_precision"]
        assert r["n"] == 12 and r["k"] == 4 and r["splits"] == 3 and 0.0 <= r["r_precision"] <= 100.0
        assert json.load(open(tmp_path / "out" / "manifest.json"))["r_precision"] == r
        gan.reset_cfg()
        capsys.readouterr()
        again = cli.main([str(tmp_path / "out"), "--cfg", yml, "--token_ids", str(tmp_path / "ids.npy"), "--per_caption", "2",
                          "--image_encoder", weights, "--text_encoder", str(tmp_path / "text.pth"), "--k", "4", "--splits", "3", "--seed", "3"])
        assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == again
        assert again == r
        gan.reset_cfg()
        assert "r_precision" not in sample.main(base)                # not asked for: the manifest of before
    finally:
        gan.reset_cfg()
        ops.set_precision("bf16")
