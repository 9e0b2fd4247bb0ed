"""Sampling on the GPU: the uint8 image kernels of csrc/image.hip against the host code they replace (`utils.visual.to_uint8_hwc`,
`make_grid` + `save_image`'s rounding), `xmc_gan_amd.infer.Sampler` against the modules called directly, and `xmc_gan/sample.py` end to end.

The bar for the kernels is EQUALITY: they restate the numpy arithmetic operation by operation in f32 (every operation rounded on its own,
correctly rounded division), so there is no tolerance to derive.  Output alignment: the kernels accept any byte address (they do not
return XMC_EALIGN for the destination): leading / trailing pixels are written one by one, the body as aligned 32-bit words; the guard
byte checks below run every shape at byte offsets 0 and 1 of a buffer."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_util import CFG_DIR
from xmc_gan.utils.visual import make_grid, to_uint8_hwc
from xmc_gan_amd import ops

DEV = torch.device("cuda", 0)
MODES = ("bf16", "f16", "fp32")
GUARD = 64


@pytest.fixture(autouse=True)
def _restore():
    yield
    ops.set_precision("bf16")
    from xmc_gan.config import gan
    gan.reset_cfg()


def _ref_u8(x8):
    """[N,H,W,8] device tensor -> uint8 [N,H,W,3] by the host code"""
    x = x8[..., :3].float().permute(0, 3, 1, 2).cpu().numpy()
    return np.stack([to_uint8_hwc(img) for img in x])


def _all_16bit_values(dtype):
    """every finite value of the 16-bit format in [-1, 1], as a tensor of that format"""
    v = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)
    v = v[torch.isfinite(v.float()) & (v.float().abs() <= 1.0)]
    assert v.numel() == {torch.bfloat16: 32514, torch.float16: 30722}[dtype]
    return v


def _filled(values_f32, dtype):
    """values in channels 0..2 of a [1,128,128,8] image (remaining slots 0), channels 3..7 = 7.0"""
    x = torch.zeros(128 * 128 * 3, dtype=torch.float32)
    assert values_f32.numel() <= x.numel()
    x[:values_f32.numel()] = values_f32
    x8 = torch.full((1, 128, 128, 8), 7.0, dtype=torch.float32)
    x8[..., :3] = x.view(1, 128, 128, 3)
    return x8.to(dtype).to(DEV)


@pytest.mark.parametrize("mode", MODES)
def test_image_to_u8_every_16bit_value(mode):
    ops.set_precision(mode)
    dt = ops.act_dtype()
    if mode == "fp32":
        g = torch.Generator().manual_seed(0)
        sets = [torch.cat((_all_16bit_values(h).float(), torch.rand(10000, generator=g) * 2 - 1)) for h in (torch.bfloat16, torch.float16)]
    else:
        sets = [_all_16bit_values(dt).float()]
    for vals in sets:
        x8 = _filled(vals, dt)
        got = ops.image_to_u8(x8).cpu().numpy()
        ref = _ref_u8(x8)
        assert got.shape == (1, 128, 128, 3) and got.dtype == np.uint8
        bad = np.flatnonzero(got != ref)
        assert bad.size == 0, (mode, bad.size, bad[:5].tolist(), got.ravel()[bad[:5]].tolist(), ref.ravel()[bad[:5]].tolist())
        flat = got.ravel()[:vals.numel()]
        assert (flat[(vals == -1.0).numpy()] == 0).all() and (flat[(vals == 1.0).numpy()] == 255).all()
        assert (vals == 1.0).any() and (vals == -1.0).any()
    # out of range input is defined: saturation, NaN -> 0
    x8 = torch.zeros((1, 1, 3, 8), dtype=torch.float32)
    x8[0, 0, :, :3] = torch.tensor([[-3.0, 3.0, float("nan")], [float("inf"), -float("inf"), 1.5], [-1.0, 1.0, 0.0]])
    got = ops.image_to_u8(x8.to(dt).to(DEV)).cpu().numpy()[0, 0]
    assert got.tolist() == [[0, 255, 0], [255, 0, 255], [0, 255, 127]]


def _guarded(nbytes, offset):
    """a 0xA5-filled buffer and the `nbytes` slice of it that starts `offset` bytes after a 4-byte boundary, GUARD bytes either side"""
    buf = torch.full((GUARD + 4 + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 4 == 0
    lo = GUARD + offset
    return buf, buf[lo:lo + nbytes], lo


def _guards_intact(buf, lo, nbytes):
    b = buf.cpu().numpy()
    return (b[:lo] == 0xA5).all() and (b[lo + nbytes:] == 0xA5).all()


def _random_images(N, H, W, dt, seed):
    g = torch.Generator().manual_seed(seed)
    x8 = torch.full((N, H, W, 8), 7.0, dtype=torch.float32)
    x8[..., :3] = torch.rand(N, H, W, 3, generator=g) * 2 - 1
    return x8.to(dt).to(DEV)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 5, 7), (3, 8, 12), (2, 64, 64)])
def test_image_to_u8_shapes_and_guard_bytes(mode, shape):
    ops.set_precision(mode)
    N, H, W = shape
    x8 = _random_images(N, H, W, ops.act_dtype(), seed=N * 100 + H)
    ref = _ref_u8(x8)
    for offset in (0, 1):
        buf, out, lo = _guarded(3 * N * H * W, offset)
        assert out.data_ptr() % 4 == offset
        ret = ops.image_to_u8(x8, out=out.view(N, H, W, 3))
        assert ret.data_ptr() == out.data_ptr()
        assert np.array_equal(ret.cpu().numpy(), ref), (mode, shape, offset)
        assert _guards_intact(buf, lo, 3 * N * H * W), (mode, shape, offset)


GRID_CASES = [(1, 5, 7, 8, 2),       # one image: make_grid's special case, no padding
              (5, 9, 11, 8, 2),      # one partial row
              (11, 8, 8, 4, 2),      # three rows, the last one partial: empty cells
              (3, 64, 64, 2, 0),     # no padding
              (2, 40, 40, 8, 2)]     # more than one (min, max) partial per image


def _grid_images(N, H, W, dt, seed):
    """random images of different ranges; from two images on the last one is constant (hi == lo), from three on image 1 has a range of 1e-6"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(N, H, W, 3, generator=g) * 2 - 1) * (0.2 + 0.8 * torch.rand(N, 1, 1, 1, generator=g)) + 0.1 * torch.randn(N, 1, 1, 1, generator=g)
    if N >= 2:
        x[N - 1] = 0.25
    if N >= 3:
        x[1] = torch.randint(0, 5, (H, W, 3), generator=g).float() * 2.5e-7
        x[1, 0, 0, 0], x[1, -1, -1, 2] = 0.0, 1e-6
    x8 = torch.full((N, H, W, 8), 7.0, dtype=torch.float32)
    x8[..., :3] = x
    return x8.to(dt).to(DEV)


def _ref_grid(x8, nrow, padding):
    x = x8[..., :3].float().permute(0, 3, 1, 2).cpu().numpy()
    return np.clip(make_grid(x, nrow, padding) * 255.0 + 0.5, 0, 255).astype(np.uint8).transpose(1, 2, 0)      # what save_image encodes


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", GRID_CASES)
def test_image_grid_u8_equals_save_image(mode, case):
    ops.set_precision(mode)
    N, H, W, nrow, padding = case
    x8 = _grid_images(N, H, W, ops.act_dtype(), seed=N + H)
    ref = _ref_grid(x8, nrow, padding)
    if N >= 3:
        xf = x8[1, ..., :3].float()
        assert 0 < float(xf.max() - xf.min()) < 2e-6
    got = ops.image_grid_u8(x8, nrow=nrow, padding=padding)
    assert tuple(got.shape) == ref.shape and got.dtype == torch.uint8
    diff = np.argwhere(got.cpu().numpy() != ref)
    assert diff.size == 0, (mode, case, len(diff), diff[:5].tolist())
    for offset in (0, 1):
        buf, out, lo = _guarded(ref.size, offset)
        ops.image_grid_u8(x8, nrow=nrow, padding=padding, out=out.view(ref.shape))
        assert np.array_equal(out.view(ref.shape).cpu().numpy(), ref), (mode, case, offset)
        assert _guards_intact(buf, lo, ref.size), (mode, case, offset)


def test_image_ops_refuse_bad_device_tensors():
    x = torch.zeros((1, 4, 4, 8), dtype=torch.bfloat16, device=DEV)
    for fn in (ops.image_to_u8, ops.image_grid_u8):
        with pytest.raises(ValueError):
            fn(torch.zeros((1, 4, 4, 16), dtype=torch.bfloat16, device=DEV))
        with pytest.raises(ValueError):
            fn(x.clone().requires_grad_())
        with pytest.raises(TypeError):
            fn(x.float())                       # an f32 image in the bf16 mode
        with pytest.raises(ValueError):
            fn(x, out=torch.zeros(5, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.image_grid_u8(x, nrow=0)


# ------------------------------------------------------------------------------------------ the sampler and the command line
def _yml(tmp_dir, gen="DF_GEN"):
    """the `_mini_yml` recipe of tests/test_entrypoint_gpu.py: df_gan_damsm.yml at 64 px, thin, tiny vocabulary, no encoder file"""
    txt = open(os.path.join(CFG_DIR, "df_gan_damsm.yml")).read()
    rep = {"NCH: 32": "NCH: 8", "VOCA_SIZE: 27297": "VOCA_SIZE: 40", "BATCH_SIZE: 88": "BATCH_SIZE: 4", "LOG_INTERVAL: 200": "LOG_INTERVAL: 2",
           "NUM_WORKERS: 8": "NUM_WORKERS: 0", "ENCODER_DIR: data/DAMSMencoders/coco/text_encoder100.pth": "ENCODER_DIR: ''",
           "MAX_LENGTH: 20": "MAX_LENGTH: 8", "MAGP: true": "MAGP: false", "ENCODER_NAME: DF_GEN": f"ENCODER_NAME: {gen}"}
    for a, b in rep.items():
        assert a in txt, a
        txt = txt.replace(a, b)
    path = os.path.join(str(tmp_dir), f"mini_{gen}.yml")
    with open(path, "w") as f:
        f.write(txt)
    return path


def _use_cfg(yml):
    from xmc_gan.config import gan
    gan.reset_cfg()
    gan.cfg_from_file(yml)
    return gan.cfg


def _text_inputs(cfg, lengths, seed):
    """what a text encoder hands the loop: words_embs [B,E,T], sent_embs [B,E], mask [B,T] (True = padding), captions of different lengths"""
    g = torch.Generator().manual_seed(seed)
    B, E, T = len(lengths), cfg.TEXT.EMBEDDING_DIM, cfg.TEXT.MAX_LENGTH
    words, sent = torch.randn(B, E, T, generator=g), torch.randn(B, E, generator=g)
    mask = torch.arange(T)[None, :] >= torch.tensor(lengths)[:, None]
    return words.to(DEV), sent.to(DEV), mask.to(DEV)


@pytest.mark.parametrize("gen", ["DF_GEN", "CONCEPT_OUTATTN_GEN"])
def test_sampler_images_equal_the_module(tmp_path, gen):
    import xmc_gan.train_gan as tg
    from xmc_gan_amd.infer import Sampler, truncated_noise
    cfg = _use_cfg(_yml(tmp_path, gen))
    torch.manual_seed(3)
    netG, netD, optG, optD = tg.build_models(DEV)
    words, sent, mask = _text_inputs(cfg, [8, 5, 3, 6, 2], seed=4)
    noise = truncated_noise(5, cfg.TRAIN.NOISE_DIM, seed=5)
    netG.train()
    before = {k: v.detach().clone() for k, v in netG.state_dict().items()}
    got = Sampler(netG).images(noise, sent, words, mask, micro_batch=2)                   # chunks of 2 + 2 + 1
    assert got.dtype == torch.uint8 and tuple(got.shape) == (5, 64, 64, 3) and got.is_cuda
    assert netG.training                                                                 # put back
    assert all(p.grad is None for p in netG.parameters())
    assert all(torch.equal(v, before[k]) for k, v in netG.state_dict().items())
    # the module called directly over the same chunks.  In `ops.fixed_order()`, as the sampler runs it: outside it the word-attention
    # generator's GroupNorm statistics are summed by atomics in arrival order and two forwards of the SAME inputs differ in their last
    # bits (a pixel near a truncation boundary then moves by one), so "bit for bit" has a meaning only there.  DF_GEN has no such sum.
    netG.eval()
    with torch.no_grad(), ops.fixed_order():
        ref = [netG(noise=noise[i:i + 2].to(DEV), sent_embs=sent[i:i + 2], words_embs=words[i:i + 2], mask=mask[i:i + 2]) for i in (0, 2, 4)]
    ref = np.stack([to_uint8_hwc(img) for img in torch.cat(ref)])
    diff = np.argwhere(got.cpu().numpy() != ref)
    print(f"\n[{gen}] sampler vs module: {len(diff)} of {ref.size} bytes differ")
    assert len(diff) == 0, diff[:5].tolist()
    assert torch.equal(Sampler(netG).images(noise, sent, words, mask, micro_batch=2), got)      # and a second run repeats the first
    assert len(np.unique(ref)) > 4                                                       # (not a blank image)
    # an evaluation-mode generator stays in evaluation mode
    Sampler(netG).images(noise[:1], sent[:1], words[:1], mask[:1])
    assert not netG.training
    # the engine is as it was: a training iteration runs
    netG.train()
    netD.train()
    imgs = torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(6)).to(DEV) * 2 - 1
    out = tg.gan_iteration(netG, netD, optG, optD, imgs, sent[:4], words[:4], mask[:4], noise[:4].to(DEV), {})
    assert {"errD", "errG"} <= set(out)
    assert all(bool(torch.isfinite(v).all()) for k, v in out.items() if k.startswith("err"))


def test_best_of_keeps_the_top_k_by_the_conditional_logit(tmp_path):
    import xmc_gan.train_gan as tg
    from xmc_gan_amd.infer import Sampler, truncated_noise
    cfg = _use_cfg(_yml(tmp_path))
    torch.manual_seed(8)
    netG, netD, _, _ = tg.build_models(DEV)
    words, sent, mask = _text_inputs(cfg, [8, 4, 6], seed=9)
    n, m, k = 3, 4, 2
    noise = truncated_noise(n * m, cfg.TRAIN.NOISE_DIM, seed=10)
    netD.train()
    imgs, scores, index, x8_kept = Sampler(netG, netD).best_of(m, k, noise, sent, words, mask, keep_engine=True)
    assert netD.training and netG.training
    assert tuple(imgs.shape) == (n, k, 64, 64, 3) and tuple(scores.shape) == (n, k) and tuple(index.shape) == (n, k)
    # the same 12 images through the modules, called directly
    netG.eval()
    netD.eval()
    sent_r = sent.repeat_interleave(m, dim=0)
    with torch.no_grad():
        img, x8 = netG(noise=noise.to(DEV), sent_embs=sent_r, words_embs=words.repeat_interleave(m, dim=0), mask=mask.repeat_interleave(m, dim=0),
                       return_nhwc=True)
        psent = sent_r if cfg.DISC.SEPERATE else netG.proj_sent(sent_r.float())
        logit = netD.COND_DNET(netD(None, nhwc8=x8), psent)[0].float().reshape(n, m)
    top, idx = logit.sort(dim=1, descending=True, stable=True)
    assert float((top[:, 0] - top[:, -1]).min()) > 0                                     # (the four draws do score differently)
    assert torch.equal(index, idx[:, :k]) and torch.equal(scores, top[:, :k])
    assert bool((scores[:, 0] >= scores[:, 1]).all())
    ref = np.stack([to_uint8_hwc(im) for im in img]).reshape(n, m, 64, 64, 3)
    for c in range(n):
        for j in range(k):
            assert np.array_equal(imgs[c, j].cpu().numpy(), ref[c, int(idx[c, j])])
            assert torch.equal(x8_kept[c * k + j], x8[c * m + int(idx[c, j])])
    with pytest.raises(ValueError):
        Sampler(netG).scores(x8, sent_r)                                                 # no discriminator given


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """checkpoints of two generators (one under an EMA name) and a discriminator, a miniature captions.pickle, captions as text and as ids"""
    import xmc_gan.train_gan as tg
    from xmc_gan.config import gan
    root = tmp_path_factory.mktemp("sample")
    yml = _yml(root)
    _use_cfg(yml)
    torch.manual_seed(0)
    netG, netD, _, _ = tg.build_models(DEV)
    torch.save(netG.state_dict(), root / "netG_060.pth")
    torch.save(netD.state_dict(), root / "netD_060.pth")
    torch.manual_seed(1)
    torch.save(tg.build_models(DEV)[0].state_dict(), root / "netG_ema_007.pth")
    i2w = {i: f"w{i}" for i in range(40)}
    with open(root / "captions.pickle", "wb") as f:
        pickle.dump([[], [], i2w, {v: k for k, v in i2w.items()}], f)
    (root / "caps.txt").write_text("w3 w5 w7 w9\nW11, w12 zebra w13!\n" + " ".join(f"w{i}" for i in range(20, 32)) + "\n")
    ids = np.zeros((2, 8), dtype=np.int64)
    ids[0, :3], ids[1, :8] = [4, 9, 2], range(30, 38)
    np.save(root / "ids.npy", ids)
    gan.reset_cfg()
    return dict(root=root, yml=yml)


def _run(work, out, *extra, checkpoint="netG_060.pth"):
    import xmc_gan.sample as sample
    root = work["root"]
    return sample.main(["--cfg", work["yml"], "--checkpoint", str(root / checkpoint), "--out", str(root / out), "--data_dir", str(root)] + list(extra))


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_command_line_writes_what_the_sampler_gives(work):
    import xmc_gan.sample as sample
    import xmc_gan.train_gan as tg
    from xmc_gan_amd.infer import Sampler, truncated_noise
    root = work["root"]
    args = ("--captions", str(root / "caps.txt"), "--n_per_caption", "2", "--truncation", "0.5", "--seed", "7")
    man = _run(work, "a", *args)
    names = [f"{c:05d}_{k}.png" for c in range(3) for k in range(2)]
    assert sorted(os.listdir(root / "a")) == sorted(names + ["grid.png", "captions.txt", "manifest.json"])
    assert [(r["caption"], r["k"], r["file"]) for r in man["images"]] == [(c, k, f"{c:05d}_{k}.png") for c in range(3) for k in range(2)]
    assert man == json.load(open(root / "a" / "manifest.json"))
    assert (man["seed"], man["truncation"], man["precision"], man["grid"], man["captions"]) == (7, 0.5, "bf16", "grid.png", 3)
    assert man["checkpoint"] == str(root / "netG_060.pth") and man["cfg"] == work["yml"]
    assert open(root / "a" / "captions.txt").read().splitlines() == open(root / "caps.txt").read().splitlines()
    # the same images from the library: the noise of this seed, the embeddings the run used, a generator loaded here
    inp = sample.main.last_inputs
    cfg = _use_cfg(work["yml"])
    netG = tg._GEN_ARCH["DF_GEN"](cfg).to(DEV)
    netG.load_state_dict(torch.load(root / "netG_060.pth", map_location=DEV))
    noise = truncated_noise(6, cfg.TRAIN.NOISE_DIM, seed=7, psi=0.5)
    assert float(noise.abs().max()) <= 0.5
    rep = lambda t: t.repeat_interleave(2, dim=0)                                        # noqa: E731
    s = Sampler(netG)
    u8 = s.images(noise, rep(inp["sent_embs"]), rep(inp["words_embs"]), rep(inp["mask"])).cpu().numpy()
    for r, name in enumerate(names):
        assert np.array_equal(_png(root / "a" / name), u8[r]), name
    netG.eval()
    x8 = s.engine_images(noise, rep(inp["sent_embs"]), rep(inp["words_embs"]), rep(inp["mask"]))
    assert np.array_equal(_png(root / "a" / "grid.png"), ops.image_grid_u8(x8).cpu().numpy())
    # the same arguments: the same bytes; another seed: other images
    _run(work, "b", *args)
    for name in names + ["grid.png", "captions.txt", "manifest.json"]:
        assert (root / "a" / name).read_bytes() == (root / "b" / name).read_bytes(), name
    _run(work, "c", *args[:-1], "8", "--walk", "4", "--interp_sent", "3")
    assert not np.array_equal(_png(root / "c" / names[0]), _png(root / "a" / names[0]))
    # the latent walks of that run: one row of frames each
    for c in range(3):
        assert _png(root / "c" / f"{c:05d}_walk.png").shape == (64 + 4, 4 * 66 + 2, 3)
    assert _png(root / "c" / "00000_00001_interp.png").shape == (64 + 4, 3 * 66 + 2, 3)
    assert sorted(f for f in os.listdir(root / "c") if "interp" in f) == ["00000_00001_interp.png"]      # caption 2 has no partner


def test_command_line_other_sources_and_reranking(work):
    root = work["root"]
    # an EMA-named checkpoint loads like any other; token ids as the caption source
    man = _run(work, "ema", "--token_ids", str(root / "ids.npy"), "--seed", "7", checkpoint="netG_ema_007.pth")
    assert [r["file"] for r in man["images"]] == ["00000_0.png", "00001_0.png"]
    assert open(root / "ema" / "captions.txt").read().splitlines() == ["4 9 2", "30 31 32 33 34 35 36 37"]
    plain = _run(work, "ids", "--token_ids", str(root / "ids.npy"), "--seed", "7")
    assert _png(root / "ema" / "00000_0.png").shape == (64, 64, 3)
    assert not np.array_equal(_png(root / "ema" / "00000_0.png"), _png(root / "ids" / "00000_0.png"))    # other weights, other image
    assert plain["checkpoint"].endswith("netG_060.pth") and man["checkpoint"].endswith("netG_ema_007.pth")
    # synthetic captions, reranked: 3 draws per caption, the best 2 kept with their scores, best first; --no_png writes no image files
    man = _run(work, "best", "--synthetic", "3", "--best_of", "3", "--n_per_caption", "2", "--netD", str(root / "netD_060.pth"), "--no_png")
    assert len(man["images"]) == 6 and all(r["file"] is None and np.isfinite(r["score"]) for r in man["images"])
    for c in range(3):
        a, b = (r["score"] for r in man["images"] if r["caption"] == c)
        assert a >= b
    assert sorted(os.listdir(root / "best")) == ["captions.txt", "grid.png", "manifest.json"]
    assert _png(root / "best" / "grid.png").shape == (66 + 2, 6 * 66 + 2, 3)
    assert man["best_of"] == 3 and man["netD"].endswith("netD_060.pth")
