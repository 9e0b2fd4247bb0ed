"""CPU-only checks of the sampling feature (`xmc_gan/sample.py`, `xmc_gan_amd/infer.py`, csrc/image.hip's C ABI): the entry points are
declared, exported by both builds and validate their arguments before any launch; the latent helpers, the tokeniser, the command line's
argument checks (all of which precede the device check) and the PNG writer pool."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from golden_util import CFG_DIR, ROOT

IMAGE_ENTRY_POINTS = ("xmc_image_to_u8", "xmc_image_minmax", "xmc_image_grid_u8")


def test_header_declares_the_image_entry_points():
    hdr = open(os.path.join(ROOT, "include", "xmc_gan_hip.h")).read()
    declared = set(re.findall(r"\b(xmc_[a-z0-9_]+)\s*\(", hdr))
    assert set(IMAGE_ENTRY_POINTS) <= declared
    assert "#define XMC_ABI_VERSION 13" in hdr
    note = hdr[hdr.index("Added without a new version"):hdr.index("#define XMC_ABI_VERSION")]
    assert all(n in note for n in IMAGE_ENTRY_POINTS)


@pytest.mark.parametrize("variant", ["bf16", "f16"])
def test_both_builds_export_and_validate_the_image_entry_points(variant):
    """NULL pointer / unknown dtype -> XMC_EINVAL, a non-positive N, H, W, nrow or a negative padding -> XMC_ESHAPE, a misaligned source
    -> XMC_EALIGN; all before anything is launched, so this runs without a GPU"""
    import xmc_gan_amd.lib as L
    lib = L.load(variant)
    assert L.ABI_VERSION == 13 and lib.xmc_abi_version() == 13
    assert set(IMAGE_ENTRY_POINTS) <= set(L.EXPORTS)
    for name in IMAGE_ENTRY_POINTS:
        assert hasattr(lib, name)
    EINVAL, EALIGN, ESHAPE = -1, -2, -3
    p = ctypes.c_void_p(4096)                                       # any aligned non-NULL value; never dereferenced on these paths
    odd = ctypes.c_void_p(4096 + 8)
    for dt in (L.H16, L.F32):
        assert lib.xmc_image_to_u8(None, p, 1, 4, 4, dt, None) == EINVAL
        assert lib.xmc_image_to_u8(p, None, 1, 4, 4, dt, None) == EINVAL
        assert lib.xmc_image_minmax(None, p, 1, 4, 4, dt, None) == EINVAL
        assert lib.xmc_image_minmax(p, None, 1, 4, 4, dt, None) == EINVAL
        assert lib.xmc_image_grid_u8(None, p, p, 1, 4, 4, 8, 2, dt, None) == EINVAL
        assert lib.xmc_image_grid_u8(p, None, p, 1, 4, 4, 8, 2, dt, None) == EINVAL
        assert lib.xmc_image_grid_u8(p, p, None, 1, 4, 4, 8, 2, dt, None) == EINVAL
        for N, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4)):
            assert lib.xmc_image_to_u8(p, p, N, H, W, dt, None) == ESHAPE
            assert lib.xmc_image_minmax(p, p, N, H, W, dt, None) == ESHAPE
            assert lib.xmc_image_grid_u8(p, p, p, N, H, W, 8, 2, dt, None) == ESHAPE
        assert lib.xmc_image_grid_u8(p, p, p, 2, 4, 4, 0, 2, dt, None) == ESHAPE
        assert lib.xmc_image_grid_u8(p, p, p, 2, 4, 4, 8, -1, dt, None) == ESHAPE
        assert lib.xmc_image_to_u8(odd, p, 1, 4, 4, dt, None) == EALIGN
        assert lib.xmc_image_minmax(odd, p, 1, 4, 4, dt, None) == EALIGN
        assert lib.xmc_image_grid_u8(odd, p, p, 1, 4, 4, 8, 2, dt, None) == EALIGN
    for dt in (2, -1):
        assert lib.xmc_image_to_u8(p, p, 1, 4, 4, dt, None) == EINVAL
        assert lib.xmc_image_minmax(p, p, 1, 4, 4, dt, None) == EINVAL
        assert lib.xmc_image_grid_u8(p, p, p, 1, 4, 4, 8, 2, dt, None) == EINVAL


def test_image_ops_refuse_what_they_cannot_take():
    from xmc_gan_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.image_to_u8(torch.zeros(1, 4, 4, 8, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.image_grid_u8(torch.zeros(1, 4, 4, 8, dtype=torch.bfloat16))
    # (the remaining refusals -- last dimension, requires_grad, dtype of another mode -- need a device tensor: tests/test_sample_gpu.py)


def test_truncated_noise():
    from xmc_gan_amd.infer import truncated_noise
    plain = truncated_noise(7, 16, seed=5)
    assert plain.dtype == torch.float32 and plain.shape == (7, 16) and plain.device.type == "cpu"
    assert torch.equal(plain, torch.randn(7, 16, generator=torch.Generator().manual_seed(5)))
    z = truncated_noise(7, 16, seed=5, psi=0.7)
    assert float(z.abs().max()) <= 0.7
    assert torch.equal(z, truncated_noise(7, 16, seed=5, psi=0.7))                       # deterministic
    inside = plain.abs() <= 0.7
    assert inside.any() and not inside.all()
    assert torch.equal(z[inside], plain[inside])                                         # kept where the first draw was inside
    assert not torch.equal(z, truncated_noise(7, 16, seed=6, psi=0.7))
    assert torch.equal(truncated_noise(7, 16, seed=5, psi=100.0), plain)                 # nothing to redraw
    for bad in (0, 0.0, -1.0):
        with pytest.raises(ValueError):
            truncated_noise(2, 4, seed=1, psi=bad)


def test_slerp():
    from xmc_gan_amd.infer import slerp
    g = torch.Generator().manual_seed(0)
    a, b = torch.randn(5, 12, generator=g), torch.randn(5, 12, generator=g)
    assert torch.equal(slerp(a, b, 0.0), a) and torch.equal(slerp(a, b, 1.0), b)          # exact at the ends
    per_row = slerp(a, b, torch.tensor([0.0, 1.0, 0.0, 1.0, 0.0]))
    assert torch.equal(per_row[0], a[0]) and torch.equal(per_row[1], b[1])
    e = torch.eye(6)
    mid = slerp(e[:3], e[3:], 0.5)                                                        # orthonormal pairs: the midpoint stays on the sphere
    assert torch.allclose(mid.norm(dim=1), torch.ones(3), atol=1e-6)
    assert torch.allclose(mid, (e[:3] + e[3:]) * (0.5 ** 0.5), atol=1e-6)
    same = slerp(a, a.clone(), 0.3)
    assert torch.isfinite(same).all() and torch.allclose(same, a, atol=1e-6)
    assert torch.isfinite(slerp(a, -a, 0.5)).all() and torch.isfinite(slerp(torch.zeros(2, 4), torch.ones(2, 4), 0.5)).all()
    # between the ends the norm of unit rows stays 1 and the angle to `a` grows linearly
    an, bn = a / a.norm(dim=1, keepdim=True), b / b.norm(dim=1, keepdim=True)
    q = slerp(an, bn, 0.25)
    w = torch.acos((an * bn).sum(1))
    assert torch.allclose(q.norm(dim=1), torch.ones(5), atol=1e-5)
    assert torch.allclose(torch.acos((q * an).sum(1).clamp(-1, 1)), 0.25 * w, atol=1e-4)


def test_sent_to_index_round_trips_with_index_to_sent():
    from xmc_gan.dataset import index_to_sent, sent_to_index
    i2w = {i: f"w{i}" for i in range(40)}
    w2i = {v: k for k, v in i2w.items()}
    ids = [3, 17, 39, 1, 8]
    sent = index_to_sent(i2w, [ids])[0]
    row, n = sent_to_index(w2i, sent, 8)
    assert row.dtype == np.int64 and row.shape == (8,) and n == 5
    assert row.tolist() == ids + [0, 0, 0]
    assert index_to_sent(i2w, [row]) == [sent]
    row2, n2 = sent_to_index(w2i, "  W3, w17!  (W39) w1;w8 ", 8)                            # case and punctuation
    assert row2.tolist() == row.tolist() and n2 == 5
    row3, n3 = sent_to_index(w2i, "w3 zebra w17 crossing w39", 8)                         # unknown words dropped
    assert row3.tolist() == [3, 17, 39, 0, 0, 0, 0, 0] and n3 == 3
    row4, n4 = sent_to_index(w2i, " ".join(f"w{i}" for i in range(1, 20)), 8)             # truncated
    assert row4.tolist() == list(range(1, 9)) and n4 == 8
    for empty in ("", "zebra crossing", "?!"):
        with pytest.raises(ValueError):
            sent_to_index(w2i, empty, 8)


def _yml(tmp_path, gen="DF_GEN"):
    """the `_mini_yml` recipe of tests/test_entrypoint_gpu.py: df_gan_damsm.yml at 64 px, thin, tiny vocabulary, no encoder file"""
    txt = open(os.path.join(CFG_DIR, "df_gan_damsm.yml")).read()
    rep = {"NCH: 32": "NCH: 8", "VOCA_SIZE: 27297": "VOCA_SIZE: 40", "BATCH_SIZE: 88": "BATCH_SIZE: 4", "LOG_INTERVAL: 200": "LOG_INTERVAL: 2",
           "NUM_WORKERS: 8": "NUM_WORKERS: 0", "ENCODER_DIR: data/DAMSMencoders/coco/text_encoder100.pth": "ENCODER_DIR: ''",
           "MAX_LENGTH: 20": "MAX_LENGTH: 8", "MAGP: true": "MAGP: false", "ENCODER_NAME: DF_GEN": f"ENCODER_NAME: {gen}"}
    for a, b in rep.items():
        assert a in txt, a
        txt = txt.replace(a, b)
    path = tmp_path / f"mini_{gen}.yml"
    path.write_text(txt)
    return str(path)


def test_command_line_defaults_and_refusals(tmp_path, monkeypatch):
    """every argument / cfg check of sample.main() comes before the device check: each refusal below is reached with the device reported
    absent, and a complete command then stops at exactly that check"""
    from xmc_gan.config import gan
    import xmc_gan.sample as sample
    a = sample.parse_args(["--cfg", "c.yml", "--checkpoint", "g.pth", "--out", "o"])
    assert (a.n_per_caption, a.seed, a.truncation, a.bs, a.imsize, a.precision, a.gpu_id, a.text_encoder) == (1, 100, None, -1, -1, None, 0, None)
    assert (a.captions, a.token_ids, a.synthetic, a.best_of, a.netD, a.walk, a.interp_sent, a.no_png) == ("", "", 0, 0, "", 0, 0, False)
    with pytest.raises(SystemExit):
        sample.parse_args(["--cfg", "c.yml", "--out", "o"])                               # --checkpoint is required
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    ckpt = tmp_path / "netG_ema_007.pth"
    ckpt.write_bytes(b"")
    netd = tmp_path / "netD_007.pth"
    netd.write_bytes(b"")
    base = ["--checkpoint", str(ckpt), "--out", str(tmp_path / "out")]
    try:
        yml = _yml(tmp_path)
        with pytest.raises(SystemExit, match="exactly one caption source"):
            sample.main(["--cfg", yml] + base)
        with pytest.raises(SystemExit, match="exactly one caption source"):
            sample.main(["--cfg", yml, "--synthetic", "2", "--token_ids", str(tmp_path / "t.npy")] + base)
        with pytest.raises(SystemExit, match="--netD"):
            sample.main(["--cfg", yml, "--synthetic", "2", "--best_of", "3"] + base)
        with pytest.raises(SystemExit, match="fewer"):
            sample.main(["--cfg", yml, "--synthetic", "2", "--best_of", "2", "--n_per_caption", "3", "--netD", str(netd)] + base)
        with pytest.raises(SystemExit, match="--truncation"):
            sample.main(["--cfg", yml, "--synthetic", "2", "--truncation", "0"] + base)
        with pytest.raises(SystemExit, match="--walk"):
            sample.main(["--cfg", yml, "--synthetic", "2", "--walk", "4"] + base)          # one noise per caption: nothing to walk between
        with pytest.raises(SystemExit, match="not a file"):
            sample.main(["--cfg", yml, "--synthetic", "2", "--checkpoint", str(tmp_path / "nope.pth"), "--out", str(tmp_path / "out")])
        with pytest.raises(SystemExit, match="CONCEPT_OUTATTN_GEN"):
            sample.main(["--cfg", _yml(tmp_path, "CONCEPT_OUTATTN_GEN"), "--synthetic", "2", "--interp_sent", "3"] + base)
        gan.reset_cfg()
        # caption files are read and checked on the host as well
        np.save(tmp_path / "bad.npy", np.zeros((3, 5), dtype=np.int64))
        with pytest.raises(SystemExit, match="--token_ids"):
            sample.main(["--cfg", yml, "--token_ids", str(tmp_path / "bad.npy")] + base)
        (tmp_path / "caps.txt").write_text("zebra crossing\n")
        with pytest.raises(SystemExit, match="--captions"):
            sample.main(["--cfg", yml, "--captions", str(tmp_path / "caps.txt"), "--data_dir", str(tmp_path)] + base)      # no captions.pickle
        # a complete command: the next stop is the device check
        with pytest.raises(RuntimeError, match="needs an MI355X"):
            sample.main(["--cfg", yml, "--synthetic", "2", "--interp_sent", "3", "--best_of", "3", "--netD", str(netd)] + base)
        assert not (tmp_path / "out").exists()                                            # nothing was written on the way
    finally:
        gan.reset_cfg()


def test_png_pool_round_trip_and_error(tmp_path):
    from PIL import Image
    from xmc_gan.utils.visual import PngPool
    rng = np.random.RandomState(0)
    arrs = [rng.randint(0, 256, (5, 7, 3), dtype=np.uint8) for _ in range(20)]
    pool = PngPool()
    assert 1 <= len(pool.threads) <= 8
    for i, a in enumerate(arrs):
        pool.put(a, tmp_path / f"{i}.png")
    pool.close()
    for i, a in enumerate(arrs):
        assert np.array_equal(np.asarray(Image.open(tmp_path / f"{i}.png")), a)
    for asked, most in ((64, 8), (1, 1)):
        sized = PngPool(workers=asked)
        assert 1 <= len(sized.threads) <= most
        sized.close()
    bad = PngPool(workers=2)
    bad.put(arrs[0], tmp_path / "missing_dir" / "x.png")
    bad.put(arrs[1], tmp_path / "ok.png")
    with pytest.raises(OSError):
        bad.close()
    assert np.array_equal(np.asarray(Image.open(tmp_path / "ok.png")), arrs[1])           # the other files are still written
    with pytest.raises(RuntimeError):
        bad.put(arrs[0], tmp_path / "late.png")
