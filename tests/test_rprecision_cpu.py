"""CPU-only checks of the R-precision feature (xmc_gan_amd/rprecision.py, xmc_gan/model/encoder.py CNN_ENCODER, the C ABI of
csrc/retrieval.hip and of the additions to csrc/fid.hip): the candidate table, the split statistics, the weight loader's errors, key parity
with the restatement, the entry points' argument checks (all before any launch) and the command lines' refusals."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import damsm_ref
from golden_util import ROOT

NEW_ENTRY_POINTS = ("xmc_resize_bilinear_f32", "xmc_rprecision")


# ------------------------------------------------------------------------------------------ candidate table
def test_candidate_table():
    from xmc_gan_amd.rprecision import candidate_table
    # 40 images with 5 captions each; every image is paired with its third caption
    group = np.repeat(np.arange(40), 5)
    own = np.arange(40) * 5 + 2
    t = candidate_table(own, group, k=100, seed=3)
    assert t.dtype == np.int32 and t.shape == (40, 100)
    assert np.array_equal(t[:, 0], own)
    for n in range(40):
        assert len(set(t[n].tolist())) == 100                                  # no duplicates in a row
        assert not (group[t[n, 1:]] == n).any()                                # none from the image's own group
        assert t[n].min() >= 0 and t[n].max() < 200
    assert np.array_equal(t, candidate_table(own, group, k=100, seed=3))       # the same seed, the same table
    assert not np.array_equal(t, candidate_table(own, group, k=100, seed=4))
    # groups that are not contiguous in the caption list, several images per caption
    group2 = np.array([2, 0, 1, 0, 2, 1, 3, 3])
    own2 = np.array([0, 0, 3, 6, 5])
    t2 = candidate_table(own2, group2, k=4, seed=0)
    for n in range(5):
        assert t2[n, 0] == own2[n] and len(set(t2[n].tolist())) == 4 and not (group2[t2[n, 1:]] == group2[own2[n]]).any()
    # every caption of another group is reachable, about equally often
    seen = np.zeros(8)
    for s in range(300):
        seen[candidate_table(own2[:1], group2, k=3, seed=s)[0, 1:]] += 1
    assert seen[0] == 0 and seen[4] == 0 and (np.abs(seen[[1, 2, 3, 5, 6, 7]] - 100.0) < 30.0).all()
    # exactly k - 1 others is enough, one fewer is not
    assert sorted(candidate_table([0], [0, 1, 2, 0], k=3, seed=0)[0].tolist()) == [0, 1, 2]
    with pytest.raises(ValueError):
        candidate_table([0], [0, 1, 2, 0], k=4, seed=0)
    with pytest.raises(ValueError):
        candidate_table(own, group, k=197, seed=0)                             # 195 captions of other groups
    assert candidate_table(own, group, k=196, seed=0).shape == (40, 196)
    with pytest.raises(ValueError):
        candidate_table([4], [0, 1, 2, 0], k=2, seed=0)                        # no such caption


# ------------------------------------------------------------------------------------------ split statistics
@pytest.mark.parametrize("n,splits", [(100, 10), (103, 10), (16, 4), (7, 3), (5, 5), (9, 1)])
def test_split_statistics(n, splits):
    from xmc_gan_amd.rprecision import split_statistics
    hits = (np.random.default_rng(n).random(n) < 0.6).astype(np.int64)
    step = n // splits
    want = np.array([100.0 * hits[i * step:(i + 1) * step if i < splits - 1 else n].mean() for i in range(splits)])
    mean, std, rates = split_statistics(hits, splits)
    assert np.array_equal(rates, want) and mean == want.mean() and std == np.std(want)
    if n % splits:
        assert len(hits[(splits - 1) * step:]) == step + n % splits           # the remainder is in the last split
    with pytest.raises(ValueError):
        split_statistics(hits[:splits - 1], splits)


def test_rprecision_accumulator_refuses_bad_rows():
    from xmc_gan_amd.rprecision import RPrecision
    rp = RPrecision(k=4, splits=2)
    with pytest.raises(ValueError):
        rp.update(torch.zeros(3, 8), torch.zeros(2, 8))                        # unpaired rows need a caption_of_image
    with pytest.raises(ValueError):
        rp.update(torch.zeros(3, 8), torch.zeros(3, 12))
    with pytest.raises(ValueError):
        rp.update(torch.zeros(3, 8), torch.zeros(2, 8), [0, 1, 2])
    with pytest.raises(ValueError):
        rp.hits()
    with pytest.raises(ValueError):
        RPrecision(k=1)
    rp.update(torch.zeros(4, 8), torch.zeros(2, 8), [0, 0, 1, 1])
    rp.update(torch.zeros(2, 8), torch.zeros(2, 8))
    assert (rp.n, rp.m) == (6, 4) and np.concatenate(rp._own).tolist() == [0, 0, 1, 1, 2, 3]


# ------------------------------------------------------------------------------------------ the encoder module and its loader
def test_key_parity_with_the_restatement():
    from xmc_gan.model.encoder import CNN_ENCODER
    sd = damsm_ref.random_state_dict(1, 32)
    enc = CNN_ENCODER(32)
    own = enc.state_dict()
    assert {k: tuple(v.shape) for k, v in own.items()} == {k: tuple(v.shape) for k, v in sd.items()}
    assert len(own) == 94 * 6 + 3 and not any(k.startswith(("fc.", "AuxLogits.")) for k in own)
    assert tuple(own["emb_features.weight"].shape) == (32, 768, 1, 1) and tuple(own["emb_cnn_code.weight"].shape) == (32, 2048)
    assert enc.Mixed_5b.branch1x1.bn.eps == 1e-3 and enc.Conv2d_1a_3x3.conv.stride == (2, 2) and enc.Mixed_6b.branch7x7_2.conv.padding == (0, 3)
    enc.load_state_dict(sd, strict=True)
    enc.load_state_dict({"module." + k: v for k, v in sd.items()}, strict=True)
    assert torch.equal(enc.state_dict()["Mixed_7c.branch_pool.bn.running_var"], sd["Mixed_7c.branch_pool.bn.running_var"])
    with pytest.raises(RuntimeError):
        enc.load_state_dict({k: v for k, v in sd.items() if k != "emb_cnn_code.bias"}, strict=True)
    assert not enc.training and not any(p.requires_grad for p in enc.parameters())
    with pytest.raises(NotImplementedError):
        enc.train()
    with pytest.raises(NotImplementedError):
        enc.train(True)
    assert enc.eval() is enc and enc.train(False) is enc


def test_loader_errors(tmp_path, monkeypatch):
    from xmc_gan_amd.rprecision import ENV, load_image_encoder
    monkeypatch.delenv(ENV, raising=False)
    with pytest.raises(ImportError, match="None is given"):
        load_image_encoder(None, None, "cpu")
    with pytest.raises(ImportError, match="does not exist"):
        load_image_encoder(str(tmp_path / "nope.pth"), None, "cpu")
    sd = damsm_ref.random_state_dict(2, 32)
    path = str(tmp_path / "enc.pth")
    for missing in ("Mixed_6c.branch7x7dbl_3.bn.running_mean", "emb_features.weight", "emb_cnn_code.bias"):
        torch.save({k: v for k, v in sd.items() if k != missing}, path)
        with pytest.raises(ImportError, match=re.escape(missing)):
            load_image_encoder(path, None, "cpu")
    for key, shape in (("Mixed_5b.branch1x1.conv.weight", (64, 192, 3, 3)), ("emb_features.weight", (32, 512, 1, 1)), ("emb_cnn_code.bias", (31,)),
                       ("emb_cnn_code.weight", (32, 1024))):
        torch.save(dict(sd, **{key: torch.zeros(shape)}), path)
        with pytest.raises(ValueError, match=re.escape(key)):
            load_image_encoder(path, None, "cpu")
    torch.save(sd, path)
    with pytest.raises(ValueError, match="nef"):
        load_image_encoder(path, 64, "cpu")
    torch.save([1, 2], path)
    with pytest.raises(ImportError, match="state dict"):
        load_image_encoder(path, None, "cpu")
    # the DataParallel prefix, a file without num_batches_tracked (PyTorch < 0.4.1), extra keys, and the environment variable
    old = {"module." + k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    old["module.fc.weight"] = torch.zeros(3, 3)
    torch.save(old, path)
    monkeypatch.setenv(ENV, path)
    enc = load_image_encoder(None, None, "cpu")
    assert enc.nef == 32 and not enc.training
    got = enc.state_dict()
    assert all(torch.equal(got[k], v) for k, v in sd.items() if not k.endswith("num_batches_tracked"))


def test_restatement_pools_as_upstream_at_299():
    """upstream's avg_pool2d(kernel_size=8) on the 8x8 map of a 299x299 input is the mean over the map"""
    ref = damsm_ref.Reference(damsm_ref.random_state_dict(3, 32))
    x = torch.rand(1, 3, 299, 299, generator=torch.Generator().manual_seed(0)).double() * 2 - 1
    feats, code = ref.forward(x, 299)
    assert tuple(feats.shape) == (1, 32, 17, 17) and tuple(code.shape) == (1, 32)
    # the same through the mean: run the trunk by hand
    with torch.no_grad():
        y = x
        for n in ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"):
            y = ref.conv(n, y)
        y = F.max_pool2d(y, 3, stride=2)
        y = F.max_pool2d(ref.conv("Conv2d_4a_3x3", ref.conv("Conv2d_3b_1x1", y)), 3, stride=2)
        for m in ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7a", "Mixed_7b", "Mixed_7c"):
            y = ref.block(m, y)
        assert tuple(y.shape) == (1, 2048, 8, 8)
        by_mean = F.linear(y.mean((2, 3)), ref.sd["emb_cnn_code.weight"], ref.sd["emb_cnn_code.bias"])
    assert float((code - by_mean).abs().max()) <= 1e-13 * float(code.abs().max())
    assert float(code.abs().mean()) > 0.1                                      # codes of order 1


# ------------------------------------------------------------------------------------------ the C ABI, without a GPU
def test_header_declares_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "xmc_gan_hip.h")).read()
    declared = set(re.findall(r"\b(xmc_[a-z0-9_]+)\s*\(", hdr))
    assert set(NEW_ENTRY_POINTS) <= declared
    assert "#define XMC_ABI_VERSION 13" in hdr
    note = hdr[hdr.index("Added without a new version"):hdr.index("#define XMC_ABI_VERSION")]
    assert all(n in note for n in NEW_ENTRY_POINTS) and "XMC_POOL_AVG_PAD" in note
    assert "#define XMC_POOL_AVG_PAD 2" in hdr
    mk = open(os.path.join(ROOT, "xmc-gan_amd", "csrc", "Makefile")).read()
    assert "retrieval.hip" in mk[mk.index("SRCS"):mk.index("OBJS")]


@pytest.mark.parametrize("variant", ["bf16", "f16"])
def test_both_builds_export_and_validate_the_new_entry_points(variant):
    """NULL pointers and N, M, K < 1 -> XMC_EINVAL; D % 4 != 0 or D > 1024 -> XMC_ESHAPE; the average over 9 at stride 2 -> XMC_EINVAL; all
    before anything is launched, so this runs without a GPU"""
    import xmc_gan_amd.lib as L
    lib = L.load(variant)
    assert L.ABI_VERSION == 13 and lib.xmc_abi_version() == 13 and L.POOL_AVG_PAD == 2
    assert set(NEW_ENTRY_POINTS) <= set(L.EXPORTS)
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name)
    EINVAL, EALIGN, ESHAPE = -1, -2, -3
    p = ctypes.c_void_p(4096)                                                  # any aligned non-NULL value; never dereferenced on these paths
    odd = ctypes.c_void_p(4096 + 8)
    rp = lib.xmc_rprecision
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert rp(*args, p, 2, 2, 2, 8, None) == EINVAL
    for N, M, K in ((0, 2, 2), (2, 0, 2), (2, 2, 0), (-1, 2, 2)):
        assert rp(p, p, p, p, None, N, M, K, 8, None) == EINVAL
    for D in (6, 2, 0, -4, 1028, 1026):
        assert rp(p, p, p, p, None, 2, 2, 2, D, None) == ESHAPE
    assert rp(odd, p, p, p, None, 2, 2, 2, 8, None) == EALIGN and rp(p, odd, p, p, None, 2, 2, 2, 8, None) == EALIGN
    rs = lib.xmc_resize_bilinear_f32
    assert rs(None, p, 1, 4, 4, 8, 8, None) == EINVAL and rs(p, None, 1, 4, 4, 8, 8, None) == EINVAL
    for dims in ((0, 4, 4, 8, 8), (1, 0, 4, 8, 8), (1, 4, 0, 8, 8), (1, 4, 4, 0, 8), (1, 4, 4, 8, 0), (1, 1 << 16, 1 << 16, 8, 8)):
        assert rs(p, p, *dims, None) == ESHAPE
    assert rs(p, odd, 1, 4, 4, 8, 8, None) == EALIGN
    pool = lib.xmc_pool3x3
    assert pool(p, p, 1, 5, 5, 8, L.POOL_AVG_PAD, 2, None) == EINVAL           # the average over 9 exists at stride 1 only
    assert pool(None, p, 1, 5, 5, 8, L.POOL_AVG_PAD, 1, None) == EINVAL and pool(p, p, 1, 5, 5, 8, 3, 1, None) == EINVAL
    assert pool(p, p, 1, 5, 5, 6, L.POOL_AVG_PAD, 1, None) == EALIGN and pool(p, p, 0, 5, 5, 8, L.POOL_AVG_PAD, 1, None) == ESHAPE


def test_ops_refuse_host_tensors_and_bad_modes():
    from xmc_gan_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.rprecision(torch.zeros(2, 8), torch.zeros(2, 8), torch.zeros((2, 2), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.resize_bilinear_f32(torch.zeros(1, 3, 4, 4))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.pool3x3(torch.zeros(1, 4, 4, 8), "avg_pad", 1)


def test_trunk_variants():
    from xmc_gan_amd import fid as FID
    assert FID.VARIANTS == ("fid", "torchvision") and issubclass(FID.InceptionFID, FID.InceptionTrunk)
    with pytest.raises(ValueError):
        FID.InceptionTrunk({}, "cpu", "tf")


# ------------------------------------------------------------------------------------------ command lines
def test_command_line_refusals(tmp_path, monkeypatch):
    """every argument / cfg check comes before the device check"""
    import xmc_gan.rprecision as cli
    import xmc_gan.sample as sample
    import xmc_gan.train_gan as tg
    from test_sample_cpu import _yml
    from xmc_gan.config import gan
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.delenv("XMC_DAMSM_IMAGE_ENCODER", raising=False)
    a = sample.parse_args(["--cfg", "c.yml", "--checkpoint", "g.pth", "--out", "o"])
    assert (a.rprecision, a.damsm_image_encoder, a.rp_k, a.rp_splits) == (False, "", 100, 10)
    assert tg.parse_args(["--cfg", "c.yml"]).damsm_image_encoder == ""
    c = cli.parse_args(["d", "--cfg", "c.yml"])
    assert (c.k, c.splits, c.seed, c.per_caption, c.batch, c.image_encoder, c.text_encoder) == (100, 10, 0, 1, 100, "", None)
    ckpt, weights = tmp_path / "netG.pth", tmp_path / "image_encoder.pth"
    ckpt.write_bytes(b"")
    weights.write_bytes(b"")
    base = ["--checkpoint", str(ckpt), "--out", str(tmp_path / "out"), "--synthetic", "2"]
    try:
        yml = _yml(tmp_path)
        with pytest.raises(SystemExit, match="damsm_image_encoder"):
            sample.main(["--cfg", yml, "--rprecision"] + base)
        with pytest.raises(SystemExit, match="damsm_image_encoder"):
            sample.main(["--cfg", yml, "--rprecision", "--damsm_image_encoder", str(tmp_path / "nope.pth")] + base)
        with pytest.raises(SystemExit, match="rp_k"):
            sample.main(["--cfg", yml, "--rprecision", "--damsm_image_encoder", str(weights), "--rp_k", "1"] + base)
        sbert = os.path.join(ROOT, "xmc_gan", "cfg", "df_gan_sbert.yml")
        with pytest.raises(SystemExit, match="TEXT.ENCODER_NAME is SBERT"):
            sample.main(["--cfg", sbert, "--rprecision", "--damsm_image_encoder", str(weights)] + base)
        gan.reset_cfg()
        with pytest.raises(RuntimeError, match="needs an MI355X"):
            sample.main(["--cfg", yml, "--rprecision", "--damsm_image_encoder", str(weights)] + base)
        gan.reset_cfg()
        with pytest.raises(SystemExit, match="damsm_image_encoder"):
            tg.main(["--cfg", yml, "--synthetic", "1", "--damsm_image_encoder", str(tmp_path / "nope.pth")])
        gan.reset_cfg()
        # the scoring command line
        imgs = tmp_path / "imgs"
        imgs.mkdir()
        ids = tmp_path / "ids.npy"
        np.save(ids, np.array([[3, 4, 5, 0, 0, 0, 0, 0], [6, 7, 0, 0, 0, 0, 0, 0]], dtype=np.int64))
        full = [str(imgs), "--cfg", yml, "--token_ids", str(ids), "--image_encoder", str(weights)]
        with pytest.raises(SystemExit, match="exactly one caption source"):
            cli.main([str(imgs), "--cfg", yml, "--image_encoder", str(weights)])
        with pytest.raises(SystemExit, match="holds no image"):
            cli.main(full)
        from PIL import Image
        for i in range(3):
            Image.fromarray(np.zeros((8, 8, 3), dtype=np.uint8)).save(str(imgs / f"{i}.png"))
        with pytest.raises(SystemExit, match="image_encoder"):
            cli.main(full[:-1] + [str(tmp_path / "nope.pth")])
        with pytest.raises(SystemExit, match="--k"):
            cli.main(full + ["--k", "1"])
        with pytest.raises(SystemExit, match="not a file"):
            cli.main(full + ["--text_encoder", str(tmp_path / "nope.pth")])
        gan.reset_cfg()
        with pytest.raises(SystemExit, match="3 images, 2 captions"):
            cli.main(full)
        gan.reset_cfg()
        (imgs / "2.png").unlink()
        with pytest.raises(RuntimeError, match="MI355X"):
            cli.main(full)
    finally:
        gan.reset_cfg()
