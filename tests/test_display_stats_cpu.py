"""Display statistics, CPU side: the tests' numpy restatement
(tests/stats_ref.py) against what the reference's own CImg returns
(tests/golden/ref_display_stats.bin, written by tests/native/ref_cimg_stats.cpp),
the host layer's histogram / kth_smallest / tone_map / white_rank_for against
the same, the declared and exported symbols, and the conditions under which
the GPU tests' inputs (tests/stats_cases.py) discriminate."""
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import display_ref as dr
import stats_cases as sc
import stats_ref as sr
from ipt_amd import capi

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
REFERENCE = Path(os.environ.get("IPT_REFERENCE", "/root/reference"))


def _has_reference():
    try:
        return (REFERENCE / "include" / "CImg.h").is_file()
    except OSError:
        return False


CASES = sr.cimg_cases()


# ---- the fixture is what the reference's CImg writes ------------------------
@pytest.mark.skipif(not _has_reference(), reason="the reference tree is not present")
def test_fixture_is_reproduced_by_the_reference(tmp_path):
    exe = tmp_path / "ref_cimg_stats"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Dcimg_display=0", f"-I{REFERENCE / 'include'}",
                    str(HERE / "native" / "ref_cimg_stats.cpp"), "-o", str(exe), "-lpthread"], check=True)
    subprocess.run([str(exe), str(tmp_path / "out.bin")], check=True)
    assert (tmp_path / "out.bin").read_bytes() == sr.GOLDEN.read_bytes()


def test_fixture_is_small():
    assert sr.GOLDEN.stat().st_size < 100 * 1024
    assert max(c["W"] * c["H"] for c in CASES) <= 64 * 64


# ---- stats_ref against CImg ---------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_stats_ref_equals_cimg(case):
    px, nb, k = case["px"], case["nb"], case["k"]
    mx, lo, _, _ = sr.hist_bounds(px)
    assert dr.bits(mx) == dr.bits(case["mx"])
    hist = sr.histogram(px, nb)
    assert np.array_equal(hist, case["hist"]), np.flatnonzero(hist != case["hist"])[:5]
    assert dr.bits(sr.kth_smallest(px, k)) == dr.bits(case["kth"])
    name = case["name"]
    if name == "spread":
        assert k == 808 and int((hist > 0).sum()) >= 50
    if name in ("constant", "zeros"):
        assert hist[-1] == px.size and hist.sum() == px.size
    if name == "negative_max":
        assert lo > mx and hist.sum() == int((px == mx).sum()) and hist[0] == hist.sum()
    if name == "inf_max":
        assert hist[-1] == int(np.isinf(px).sum()) == hist.sum() and k >= px.size and np.isinf(case["kth"])
    if name == "subnormal_max":
        assert 0 < mx < np.finfo(np.float32).tiny and lo == 0
    if name == "two_valued":
        assert case["kth"] == 4.0 and sr.kth_smallest(px, k - 1) == 1.0


# ---- the host layer's restatements ------------------------------------------
@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    ge.build_lib()
    ge.build_host()
    exe = tmp_path_factory.mktemp("host") / "host_stats_dump"
    subprocess.run(["g++", *ge.GXX_FLAGS, "-o", str(exe), str(HERE / "native" / "host_stats_dump.cpp"),
                    f"-I{ge.HOST}", f"-L{ge.LIB.parent}", "-lipt_host", "-lipt_hip",
                    f"-Wl,-rpath,{ge.LIB.parent}", "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    return exe


def _run(dump, *args):
    return subprocess.run([str(dump), *map(str, args)], check=True, capture_output=True, text=True).stdout.split()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_layer_equals_cimg(dump, tmp_path, case):
    case["px"].tofile(tmp_path / "p.f32")
    W, H = case["W"], case["H"]
    hist = np.array(_run(dump, "hist", W, H, tmp_path / "p.f32", case["nb"]), np.uint32)
    assert np.array_equal(hist, case["hist"])
    kth, = _run(dump, "kth", W, H, tmp_path / "p.f32", case["k"])
    assert int(kth) == sr.bits1(case["kth"])


def test_host_layer_stated_order_and_tone(dump, tmp_path):
    """-0 before +0, NaNs after +inf (0x7fc00000), a rank past the end gives the
    maximum; tone_map(plane, white) is display_ref's arithmetic with white."""
    name, W, H, img, ranks = [c for c in sc.select_edge_cases() if c[0] == "signs_zeros_infs"][0]
    img.tofile(tmp_path / "s.f32")
    for k in ranks + (W * H + 5,):
        got, = _run(dump, "kth", W, H, tmp_path / "s.f32", k)
        assert int(got) == sr.bits1(sr.kth_smallest(img, k)), k
    name, W, H, img, ranks = [c for c in sc.select_edge_cases() if c[0] == "nans"][0]
    img.tofile(tmp_path / "n.f32")
    for k in ranks:
        got, = _run(dump, "kth", W, H, tmp_path / "n.f32", k)
        assert int(got) == sr.bits1(sr.kth_smallest(img, k)), k
    W, H, img = sc.percentile_image()
    img.tofile(tmp_path / "t.f32")
    white = sr.kth_smallest(img, sr.white_rank_for(W, H, 0.95))
    _run(dump, "tone", W, H, tmp_path / "t.f32", sr.bits1(white), tmp_path / "t.out")
    got = np.fromfile(tmp_path / "t.out", np.float32)
    assert np.array_equal(dr.bits(got), dr.bits(sr.tone_map(img, white)))


def test_white_rank_for(dump):
    for W, H, f, want in ((37, 23, 0.95, 808), (640, 640, 0.95, 389120), (64, 64, 0.5, 2048), (7, 3, 1.0, 21)):
        assert sr.white_rank_for(W, H, f) == want
        assert capi.white_rank_for(W, H, f) == want
        assert int(_run(dump, "rank", W, H, f)[0]) == want


# ---- symbols -----------------------------------------------------------------
def test_symbols_declared_and_exported():
    txt = (ROOT / "include" / "ipt_capi.h").read_text()
    assert re.search(r"#define\s+IPT_ABI_VERSION\s+7\b", txt)
    assert "typedef struct ipt_display_stats_params" in txt
    ge.build_lib()
    lib = capi.load()
    for sym in ("ipt_display_stats_device", "ipt_display_stats"):
        assert re.search(rf"^int {sym}\(", txt, re.M)
        assert sym in capi.EXPORTED_SYMBOLS
        assert hasattr(lib, sym)
    import ctypes as C
    # int32 x2, float, int32, int64, uint32 (+ tail padding)
    assert C.sizeof(capi.DisplayStatsParams) == 32
    assert capi.DisplayStatsParams.white_rank.offset == 16 and capi.DisplayStatsParams.flags.offset == 24


# ---- the GPU tests' inputs discriminate --------------------------------------
def test_spread_case_fills_buckets():
    assert int((sr.histogram(sc.spread_image(), 400) > 0).sum()) >= 50
    for nb in (1, 2, 400, 4095, 4096):
        h = sr.histogram(sc.spread_image(), nb)
        assert h.size == nb and h.sum() > 0.99 * 97 * 33


def test_percentile_case_changes_the_picture():
    W, H, img = sc.percentile_image()
    k = sr.white_rank_for(W, H, 0.95)
    ref, ref_max = sr.stats_ref(img, W, H, 0.0, 400, k), sr.stats_ref(img, W, H, 0.0, 400, -1)
    mx, _, white, _ = ref["stats"]
    assert white < mx and ref_max["stats"][2] == mx
    assert (ref["tone"] == 1.0).mean() >= 0.01
    assert (ref["gray8"] != ref_max["gray8"]).mean() > 0.5
    assert np.array_equal(ref_max["gray8"], dr.display_ref(img, W, H)["gray8"])


def test_hist_edge_cases_reach_their_branches():
    cases = {c[0]: c for c in sc.hist_edge_cases()}
    for name, (_, W, H, img, nb) in cases.items():
        assert img.size == W * H, name
        mx, lo, vmin, vmax = sr.hist_bounds(img)
        h = sr.histogram(img, nb)
        if name in ("constant", "zeros"):
            assert h[-1] == img.size and (vmin == vmax if name == "zeros" else vmin < vmax)
        elif name == "negative_max":
            assert mx < 0 and lo > mx and vmin == mx and h[0] == h.sum() == int((img == mx).sum()) > 0
        elif name == "inf_max":
            assert np.isinf(mx) and h[-1] == h.sum() == 2
        elif name == "nan_first":
            assert np.isnan(mx) and h.sum() == 0
        elif name == "nan_elsewhere":
            assert not np.isnan(mx) and np.isnan(img).sum() == 1 and h.sum() > 0.99 * img.size
        elif name == "subnormal_max":
            assert 0 < mx < np.finfo(np.float32).tiny and lo == 0 and int((h > 0).sum()) >= 50
        elif name == "inner_edges":
            # every inner edge separates the floats around it: each bucket but the outermost is hit
            assert img.size == 1 + 3 * 399 and int((h > 0).sum()) == 400
    assert {f"buckets_{nb}" for nb in (1, 2, 400, 4095, 4096)} <= set(cases)


def test_select_edge_cases_reach_their_branches():
    cases = {c[0]: c for c in sc.select_edge_cases()}
    for name, (_, W, H, img, ranks) in cases.items():
        assert img.size == W * H, name
    n = 37 * 23
    assert cases["ranks"][4] == (0, 1, n // 2, n - 2, n - 1, n, 2 * n)
    _, _, _, two, (a, b) = cases["two_valued"]
    assert sr.kth_smallest(two, a) == 1.0 and sr.kth_smallest(two, b) == 4.0
    low, high = sr.keys(cases["low_digit"][3]), sr.keys(cases["high_digit"][3])
    assert len(np.unique(low >> 10)) == 1 and len(np.unique(low)) > 100
    assert len(np.unique(high & 0x1fffff)) == 1 and len(np.unique(high >> 21)) > 100
    _, _, _, s, ranks = cases["signs_zeros_infs"]
    got = [sr.bits1(sr.kth_smallest(s, k)) for k in ranks]
    assert got[0] == 0xff800000 and got[3:7] == [0x80000000, 0x80000000, 0, 0] and got[-2:] == [0x7f800000] * 2
    _, _, _, nans, ranks = cases["nans"]
    got = [sr.bits1(sr.kth_smallest(nans, k)) for k in ranks]
    assert np.isnan(nans).sum() == 40 and (dr.bits(nans) >> 31)[np.isnan(nans)].any()
    assert got[1] == sr.bits1(nans[~np.isnan(nans)].max()) and got[2:] == [0x7fc00000] * 3
    _, _, _, img, (first, last) = cases["bin_edges"]
    tf, tl = sc.select_trace(img, first), sc.select_trace(img, last)
    assert [r for r, c in tf] == [0, 0, 0] and all(c > 1 for r, c in tf)
    assert all(r == c - 1 for r, c in tl) and all(c > 1 for r, c in tl) and tl[0][1] > 300


def test_shape_inputs_have_glare_work_and_a_percentile():
    for W, H in ((37, 23), (640, 640)):
        img = sc.shape_image(W, H)
        assert 0 < int((img > sc.CUTOFF).sum()) <= 12
    assert {(640, 640), (257, 1024), (4096, 512), (1024, 1024), (1, 1)} <= set(sc.SHAPES)
    img, k, ref = sc.shape_ref(37, 23, False)
    assert k == 808 and ref["stats"][2] < ref["stats"][0]
