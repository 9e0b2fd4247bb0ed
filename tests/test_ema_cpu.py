"""The generator weight average (EMA), the parts that need no GPU: the entry point's flags, the C ABI's declarations and the
argument validation of the two entry points (which happens before anything is launched)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("xmc_ema_step", "xmc_optim_step")


def test_flags_default_off_and_parse():
    import xmc_gan.train_gan as tg
    a = tg.parse_args([])
    assert a.ema_decay == 0.0 and a.ema_start == 0
    # the reference's seven flags keep their defaults
    assert (a.cfg, a.gpu_id, a.seed, a.resume_epoch, a.log_type, a.bs, a.imsize) == \
        ('xmc_gan/cfg/df_gan_sbert_seperate.yml', 0, 100, 0, 'tb', -1, -1)
    b = tg.parse_args(["--ema_decay", "0.999", "--ema_start", "2000"])
    assert b.ema_decay == 0.999 and b.ema_start == 2000
    assert tg.StepOptions().ema is None
    for bad in (["--ema_decay", "1.0"], ["--ema_decay", "-0.1"], ["--ema_decay", "0.9", "--ema_start", "-1"]):
        with pytest.raises(SystemExit):
            tg.main(bad)                         # rejected before the cfg is read or a device is touched


def test_header_declares_the_entry_points_and_binding_mirrors_them(tmp_path):
    import xmc_gan_amd.lib as L
    hdr_path = os.path.join(ROOT, "include", "xmc_gan_hip.h")
    hdr = open(hdr_path).read()
    declared = set(re.findall(r"\b(xmc_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, name
        assert name in L._SIGS and name in L.EXPORTS, name
    assert "typedef struct XmcEmaEntry" in hdr
    assert "#define XMC_ABI_VERSION 13" in hdr and L.ABI_VERSION == 13
    assert ctypes.sizeof(L.AdamEntry) == 48
    # argument counts of the binding against the declarations
    for name in NEW:
        args = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S).group(1)
        assert len(args.split(",")) == len(L._SIGS[name]), name
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    subprocess.run(["gcc", "-x", "c", "-std=c99", "-fsyntax-only", "-Wall", "-Werror", hdr_path], check=True)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "xmc_gan_hip.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(XmcEmaEntry), sizeof(XmcAdamEntry), sizeof(XmcOptimStep)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    ema_sz, adam_sz, optim_sz = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert int(ema_sz) == ctypes.sizeof(L.EmaEntry) == 24 and int(adam_sz) == ctypes.sizeof(L.AdamEntry)
    assert int(optim_sz) == ctypes.sizeof(L.OptimStep)


@pytest.mark.parametrize("variant", ["bf16", "f16"])
def test_entry_points_reject_bad_arguments_before_launching(variant):
    import xmc_gan_amd.lib as L
    lib = L.load(variant)
    for name in NEW:
        assert hasattr(lib, name), name
    one = ctypes.c_void_p(8)                     # any non-NULL value; never dereferenced on these paths
    EINVAL = -1

    def ema(tab=one, nt=1, ch=one, nc=1, decay=0.9, start=0, nupd=one):
        return lib.xmc_ema_step(tab, nt, ch, nc, decay, start, nupd, None, 1, None)

    def optim(tab=one, etab=one, nt=1, ch=one, nc=1, sf=None, si=None, mode=2, interval=1, decay=0.9, start=0, nupd=one, gs=1.0):
        s = L.OptimStep(table=tab, ema_table=etab, chunks=ch, ntensors=nt, nchunks=nc, lr=1e-4, beta1=0.0, beta2=0.9, eps=1e-8,
                        grad_scale=gs, scale_dev=sf, flags_dev=si, mode=mode, growth=2.0, backoff=0.5, interval=interval,
                        decay=decay, start=start, num_updates_dev=nupd, bump=1)
        return lib.xmc_optim_step(ctypes.byref(s), None)

    def fused(**kw):                             # Adam with the shadow update, no loss scale
        return optim(**kw)

    def scaled(sf=one, si=one, mode=7, **kw):    # ... under the dynamic loss scale
        return optim(sf=sf, si=si, mode=mode, **kw)

    for fn in (ema, fused, scaled):
        assert fn(tab=None) == EINVAL and fn(ch=None) == EINVAL and fn(nupd=None) == EINVAL
        assert fn(nt=0) == EINVAL and fn(nc=0) == EINVAL
        assert fn(decay=1.0) == EINVAL and fn(decay=-0.5) == EINVAL and fn(decay=float("nan")) == EINVAL
        assert fn(start=-1) == EINVAL
    assert fused(etab=None) == EINVAL and scaled(etab=None) == EINVAL
    assert scaled(sf=None) == EINVAL and scaled(si=None) == EINVAL and scaled(mode=0) == EINVAL and scaled(interval=0) == EINVAL
    # the same without a shadow set (ema_table and counter both NULL)
    plain = dict(etab=None, nupd=None)
    assert optim(tab=None, **plain) == EINVAL and optim(ch=None, **plain) == EINVAL
    assert optim(nt=0, **plain) == EINVAL and optim(nc=0, **plain) == EINVAL
    assert scaled(sf=None, **plain) == EINVAL and scaled(si=None, **plain) == EINVAL
    assert scaled(mode=0, **plain) == EINVAL and scaled(interval=0, **plain) == EINVAL
    # what the one entry adds: the loss scale excludes a grad_scale, and phases other than the update need the loss scale
    assert scaled(gs=0.5) == EINVAL and scaled(gs=0.5, **plain) == EINVAL
    assert all(optim(mode=m) == EINVAL and optim(mode=m, **plain) == EINVAL for m in (0, 1, 3, 4, 7))
    assert lib.xmc_optim_step(None, None) == EINVAL


def test_param_ema_rejects_bad_settings_and_has_no_cpu_fallback():
    import torch
    from xmc_gan_amd.optim import ParamEMA
    m = torch.nn.Linear(3, 2)
    for decay, start in ((1.0, 0), (-0.1, 0), (0.9, -1)):
        with pytest.raises(ValueError):
            ParamEMA(m, decay, start)
    ema = ParamEMA(m, 0.9, 2)
    sd = ema.state_dict()
    assert set(sd) == {"shadow", "num_updates", "decay", "start"} and set(sd["shadow"]) == {"weight", "bias"}
    assert sd["num_updates"] == 0 and sd["decay"] == 0.9 and sd["start"] == 2
    assert all(torch.equal(sd["shadow"][k], v) for k, v in m.state_dict().items())
    assert not any(isinstance(e, torch.nn.Parameter) for e in ema.shadow)
    with pytest.raises(RuntimeError, match="GPU only"):
        ema.update()                             # a missing device is an error, not an eager-PyTorch update
