"""csrc/conv_plan.h on the CPU: the halo plans of the convolution launchers are integer arithmetic on XmcConvDesc, so a stand-alone C++
program (plain g++, -Wall -Werror, address + undefined-behaviour sanitizers where this g++ links them) plans a handful of hand-written
descriptors and prints the plans.  What is expected is worked out here from the tap lists this file wrote: min / max of the offsets,
TH * TW == 256, tiles = map / tile -- not from how the product builds its taps."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xmc-gan_amd", "csrc")

T3 = [(h, w) for h in (-1, 0, 1) for w in (-1, 0, 1)]                      # 3x3, pad 1
T4S2 = [(h, w) for h in (-1, 0, 1, 2) for w in (-1, 0, 1, 2)]             # 4x4, stride 2, pad 1
# the data gradient of a 4x4 stride-2 layer: output parity (py, px) reads the 2x2 taps {py - 1, py} x {px - 1, px}
T2CLS = [[(py - 1 + a, px - 1 + b) for a in (0, 1) for b in (0, 1)] for py in (0, 1) for px in (0, 1)]


def desc(taps, N=2, M=(16, 16), S=None, D=None, CS=64, CD=128, CDw=None, SA=1, DA=1, **kw):
    """One descriptor: `taps` is a tap list (one class) or a list of them; maps default to the size of the GEMM grid."""
    classes = taps if isinstance(taps[0], list) else [taps]
    f = dict(N=N, MH=M[0], MW=M[1], SH=(S or M)[0], SW=(S or M)[1], DH=(D or M)[0], DW=(D or M)[1], CS=CS, CD=CD, CDw=CDw or CD, SA=SA, DA=DA,
             ntaps=len(classes[0]), nclass=len(classes), dtype="XMC_BF16", out_dtype="XMC_BF16")
    f.update(kw)
    return dict(fields=f, classes=classes)


CASES = {
    "c3_16x16": desc(T3),
    "c3_8x32": desc(T3, M=(8, 32)),
    "cls2x2": desc(T2CLS, CS=128, D=(32, 32), DA=2, dph=[0, 0, 1, 1], dpw=[0, 1, 0, 1]),
    "s2_natural": desc(T4S2, CS=128, S=(32, 32), SA=2),
    "s2_reversed": desc(T4S2[::-1], CS=128, S=(32, 32), SA=2),
    "s2_duplicate": desc(T4S2[:5] + [T4S2[3]] + T4S2[6:], CS=128, S=(32, 32), SA=2),
    "no_w24": desc(T3, M=(16, 24)),
    "no_cs96": desc(T3, CS=96),
    "no_halo17": desc(T3[:8] + [(17, 0)]),
    "halo16": desc(T3[:8] + [(16, 0)]),                                       # ... and the deepest halo a 16-row tile takes
    "no_2g_source": desc(T3, N=65536, M=(64, 64), CD=64, CDw=128),            # N * SH * SW * CS / 8 == 2^31
    "below_2g": desc(T3, N=65535, M=(64, 64), CD=64, CDw=128),
    "no_pool_odd": desc(T3, D=(17, 16), dst_pool="&pool_target"),
    "pool_even": desc(T3, dst_pool="&pool_target"),
}

MAIN = r"""
#include <stdio.h>
#include <string.h>
#include "conv_plan.h"

static char pool_target;

static void report(const char* name, const XmcConvDesc* d) {
    XmcHaloPlan t;
    memset(&t, 0, sizeof t);
    int mode = -1;
    const int ok = xmc_halo_plan(d, &t, &mode, 1);
    printf("%s ok %d same %d within1 %d", name, ok, (int)xmc_same_size_maps(d), (int)xmc_taps_within(d, 0, 1));
    for (int z = 0; z < d->nclass; ++z) {
        const XmcTapBox b = xmc_tap_box(d, z);
        printf(" box%d %d,%d,%d,%d", z, b.hmin, b.hmax, b.wmin, b.wmax);
    }
    if (ok) {
        printf(" mode %d tile %d,%d,%d tiles %d,%d nslab %d maxpatch %d", mode, t.TH, t.TW, t.log2TW, t.tiles_y, t.tiles_x, t.nslab, xmc_halo_max_patch(d, &t));
        for (int z = 0; z < d->nclass; ++z) printf(" patch%d %d,%d,%d,%d", z, t.PH[z], t.PW[z], t.dh0[z], t.dw0[z]);
        if (mode == 1) {
            printf(" tsel ");
            for (int i = 0; i < 16; ++i) printf("%d%s", t.tsel[i / 4][i % 4], i < 15 ? "," : "");
        }
    }
    printf("\n");
}

int main() {
    XmcConvDesc d;
@CASES@
    return 0;
}
"""


def _program():
    out = []
    for name, c in CASES.items():
        out.append("    memset(&d, 0, sizeof d);")
        for k, v in c["fields"].items():
            if isinstance(v, list):
                out += [f"    d.{k}[{i}] = {x};" for i, x in enumerate(v)]
            else:
                out.append(f"    d.{k} = {v};")
        for z, taps in enumerate(c["classes"]):
            for k, (h, w) in enumerate(taps):
                out.append(f"    d.dh[{z}][{k}] = {h}; d.dw[{z}][{k}] = {w}; d.wi[{z}][{k}] = {k};")
        out.append(f'    report("{name}", &d);')
    return MAIN.replace("@CASES@", "\n".join(out))


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("conv_plan")
    src, exe = tmp / "plans.cpp", tmp / "plans"
    src.write_text(_program())
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++", *san, str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode != 0:
        san = []                                # this g++ has no sanitizer runtimes to link
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *san, "-I", CSRC, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    res = {}
    for line in r.stdout.splitlines():
        tok = line.split()
        res[tok[0]] = {k: [int(x) for x in v.split(",")] for k, v in zip(tok[1::2], tok[2::2])}
    assert set(res) == set(CASES)
    return res


def _box(taps):
    hs, ws = [h for h, _ in taps], [w for _, w in taps]
    return [min(hs), max(hs), min(ws), max(ws)]


def _check_unit_stride(p, case, tile):
    """mode 0: per-class boxes, offsets and patches from the tap lists; the tile is what the issue names for the map"""
    f, TH, TW = case["fields"], tile[0], tile[1]
    assert p["ok"] == [1] and p["mode"] == [0]
    assert TH * TW == 256 and p["tile"] == [TH, TW, {16: 4, 32: 5}[TW]]
    assert p["tiles"] == [f["MH"] // TH, f["MW"] // TW] and f["MH"] % TH == 0 and f["MW"] % TW == 0
    assert p["nslab"] == [f["CS"] // 64]
    biggest = 0
    for z, taps in enumerate(case["classes"]):
        hmin, hmax, wmin, wmax = _box(taps)
        assert p[f"box{z}"] == [hmin, hmax, wmin, wmax]
        assert p[f"patch{z}"] == [TH + hmax - hmin, TW + wmax - wmin, hmin, wmin]
        biggest = max(biggest, (TH + hmax - hmin) * (TW + wmax - wmin))
    assert p["maxpatch"] == [biggest]


def test_3x3_on_a_16x16_map(plans):
    p = plans["c3_16x16"]
    _check_unit_stride(p, CASES["c3_16x16"], (16, 16))
    assert p["patch0"] == [18, 18, -1, -1] and p["nslab"] == [1] and p["tiles"] == [1, 1]
    assert p["same"] == [1] and p["within1"] == [1]


def test_3x3_on_an_8x32_map(plans):
    p = plans["c3_8x32"]
    _check_unit_stride(p, CASES["c3_8x32"], (8, 32))
    assert p["patch0"] == [10, 34, -1, -1]


def test_four_classes_of_2x2_taps(plans):
    p = plans["cls2x2"]
    _check_unit_stride(p, CASES["cls2x2"], (16, 16))
    assert [p[f"patch{z}"] for z in range(4)] == [[17, 17, -1, -1], [17, 17, -1, 0], [17, 17, 0, -1], [17, 17, 0, 0]]
    assert p["nslab"] == [2] and p["same"] == [0]              # the destination is the 32 x 32 map


@pytest.mark.parametrize("name", ["s2_natural", "s2_reversed"])
def test_4x4_stride_2_tap_selection(plans, name):
    p, case = plans[name], CASES[name]
    taps, f = case["classes"][0], case["fields"]
    assert p["ok"] == [1] and p["mode"] == [1]
    assert p["tile"] == [16, 16, 4] and p["tiles"] == [1, 1]
    assert p["nslab"] == [4 * f["CS"] // 64]
    assert p["patch0"] == [17, 17, 0, 0] and p["maxpatch"] == [17 * 17]
    tsel = p["tsel"]
    assert sorted(tsel) == list(range(16))
    for g in range(4):                          # slab group (dy, dx) of the space-to-depth view, tap (ta, tb) of its dense 2x2
        for tp in range(4):
            assert taps[tsel[4 * g + tp]] == (2 * (tp >> 1) + (g >> 1) - 1, 2 * (tp & 1) + (g & 1) - 1)
    assert p["same"] == [0] and p["within1"] == [0]


def test_4x4_stride_2_refuses_a_duplicated_tap(plans):
    assert plans["s2_duplicate"]["ok"] == [0]


@pytest.mark.parametrize("name", ["no_w24", "no_cs96", "no_halo17", "no_2g_source", "no_pool_odd"])
def test_refusals(plans, name):
    assert plans[name]["ok"] == [0]


def test_neighbours_of_the_refusals_are_planned(plans):
    """each bound sits where the refusal cases say: one row less of halo, one image less, an even pooled map"""
    p = plans["halo16"]
    assert p["ok"] == [1] and p["box0"] == [-1, 16, -1, 1] and p["patch0"] == [16 + 17, 18, -1, -1] and p["within1"] == [0]
    assert plans["below_2g"]["ok"] == [1] and plans["below_2g"]["tile"] == [8, 32, 5] and plans["below_2g"]["tiles"] == [8, 2]
    assert plans["pool_even"]["ok"] == [1]
    assert plans["no_halo17"]["box0"] == [-1, 17, -1, 1]
