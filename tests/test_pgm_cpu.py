"""PGM path, CPU side: ipt_math.h's logf_ (the library's host build,
ipt_logf_host) against the host libm over the PGM chain's whole domain, the
tests' numpy restatement (tests/pgm_ref.py) against the host layer's compiled
ipt::n_val / write_pgm (tests/native/pgm_dump.cpp) and against the compiled
reference's smooth (tests/golden/ref_smooth.bin), and the declared, bound and
exported symbols. Every comparison is bit for bit."""
import ctypes as C
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import display_ref as dr
import pgm_ref as pr
from ipt_amd import capi

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
EXHAUSTIVE = os.environ.get("IPT_EXHAUSTIVE") == "1"
CHUNK = 1 << 24


@pytest.fixture(scope="module", autouse=True)
def _lib():
    ge.build_lib()


def _assert_logf(x):
    a, b = dr.bits(capi.logf_host(x)), dr.bits(pr.libm_logf(x))
    bad = a != b
    assert not bad.any(), (int(bad.sum()), dr.bits(x)[bad][:5], a[bad][:5], b[bad][:5])


def _logf_sweep(lo, hi, stride):
    for s in range(lo, hi + 1, CHUNK * stride):
        _assert_logf(pr.floats(s, min(hi, s + CHUNK * stride - 1), stride))


# ---- 1. logf_ against libm ----------------------------------------------------
def test_logf_host_equals_libm_up_to_the_contrast():
    """Every float of [1, 500], n_val's whole domain at the reference's contrast."""
    assert pr.B500 - pr.ONE + 1 == 75_104_257
    _logf_sweep(pr.ONE, pr.B500, 1)


def test_logf_host_equals_libm_above_the_contrast():
    """Every 61st pattern of (500, FLT_MAX] and the edges."""
    _logf_sweep(pr.B500 + 1, pr.FLT_MAX, 61)
    edges = pr.logf_edges()
    assert edges.size == 6 + 64 and edges.min() == 1.0 and dr.bits(edges).max() == pr.FLT_MAX
    _assert_logf(edges)
    assert dr.bits(capi.logf_host(np.array([1.0], np.float32)))[0] == 0  # +0


def test_logf_outside_the_domain_is_the_stated_nan():
    x = np.array([0x3f7fffff, 0, 0x80000000, 0x00000001, 0xbf800000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001,
                  0x7f800001], np.uint32).view(np.float32)
    assert (dr.bits(capi.logf_host(x)) == 0x7fc00000).all()
    lib = capi.load()
    out = np.zeros(1, np.float32)
    assert lib.ipt_logf_host(None, out.ctypes.data, 1) == capi.IPT_E_INVALID
    assert lib.ipt_logf_host(out.ctypes.data, None, 1) == capi.IPT_E_INVALID
    assert lib.ipt_logf_host(out.ctypes.data, out.ctypes.data, -1) == capi.IPT_E_INVALID
    assert lib.ipt_logf_host(out.ctypes.data, out.ctypes.data, 0) == capi.IPT_OK


if EXHAUSTIVE:  # IPT_EXHAUSTIVE=1, as in tests/test_math_exhaustive.py
    @pytest.mark.slow
    def test_logf_host_equals_libm_exhaustive():
        """All 1 065 353 216 floats of [1, FLT_MAX]."""
        _logf_sweep(pr.ONE, pr.FLT_MAX, 1)


# ---- 2. pgm_ref against the host layer's compiled n_val / write_pgm ------------
@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    ge.build_host()
    exe = tmp_path_factory.mktemp("host") / "pgm_dump"
    subprocess.run(["g++", *ge.GXX_FLAGS, "-o", str(exe), str(HERE / "native" / "pgm_dump.cpp"),
                    f"-I{ge.HOST}", f"-L{ge.LIB.parent}", "-lipt_host", "-lipt_hip",
                    f"-Wl,-rpath,{ge.LIB.parent}", "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    return exe


def _b(v):
    return int(np.array([v], np.float32).view(np.uint32)[0])


def _dump_nval(dump, tmp_path, v, mx, contrast, gamma):
    v = np.ascontiguousarray(v, np.float32)
    v.tofile(tmp_path / "v.f32")
    out = subprocess.run([str(dump), "nval", str(tmp_path / "v.f32"), str(v.size), str(_b(mx)), str(_b(contrast)),
                          str(_b(gamma))], check=True, capture_output=True, text=True).stdout.split()
    return np.array(out, np.int64)


def test_n_val_table(dump, tmp_path):
    """The issue's table of odd inputs: the stated numbers, pgm_ref and the
    compiled ipt::n_val agree."""
    vals = np.array(pr.TABLE_VAL, np.float32)
    for mx in pr.TABLE_MAX:
        want = np.array(pr.table_want(mx))
        got = _dump_nval(dump, tmp_path, vals, mx, 500.0, 0.6)
        assert np.array_equal(got, want), (mx, got)
        assert np.array_equal(pr.n_val(vals, mx), want), (mx, pr.n_val(vals, mx))


@pytest.mark.parametrize("contrast,gamma", pr.PAIRS)
@pytest.mark.parametrize("W,H", [(37, 23), (300, 9)])
def test_pgm_ref_equals_host_layer(dump, tmp_path, W, H, contrast, gamma):
    img = pr.random_plane(W, H, W)
    mx = pr.fold_max0(img)
    ref = pr.n_val(img, mx, contrast, gamma)
    assert np.array_equal(_dump_nval(dump, tmp_path, img, mx, contrast, gamma), ref)
    if contrast == 500.0:
        assert ref.max() == 255 and len(np.unique(ref)) > 100 and (ref == 0).any()
    # the file: write_pgm and write_pgm_bytes print the same text
    img.tofile(tmp_path / "p.f32")
    ref.tofile(tmp_path / "p.u8")
    subprocess.run([str(dump), "pgm", str(W), str(H), str(tmp_path / "p.f32"), str(_b(mx)), str(_b(contrast)),
                    str(_b(gamma)), str(tmp_path / "a.pgm")], check=True)
    subprocess.run([str(dump), "bytes", str(W), str(H), str(tmp_path / "p.u8"), str(tmp_path / "b.pgm")], check=True)
    a = (tmp_path / "a.pgm").read_bytes()
    assert a == (tmp_path / "b.pgm").read_bytes()
    head = a.split(b"\n", 3)
    assert head[:3] == [b"P2", f"{W} {H}".encode(), b"255"]
    assert np.array_equal(np.array(head[3].split(), np.int64), ref)


# ---- 3. pgm_ref's smooth against the compiled reference -----------------------
def test_smooth_ref_equals_reference_fixture():
    cases = pr.smooth_golden_cases()
    assert len(cases) == 6
    for W, H, side, inp, sm, mx_s, mx_c in cases:
        got, mx = pr.smooth(inp, W, H, side)
        assert np.array_equal(dr.bits(got), dr.bits(sm)), (W, H, side)
        assert _b(mx) == _b(mx_s), (W, H, side)
        # computeSmoothedMax(side) of the unsmoothed plane is the same window maximum
        assert _b(mx) == _b(mx_c), (W, H, side)
        # main.cpp's sequence: the window maximum of the smoothed plane decides
        ref = pr.pgm_ref(inp, W, H, side, 5)
        assert _b(ref["stats"][0]) == _b(pr.smooth(sm, W, H, 5)[1])


# ---- 4. header and binding -------------------------------------------------------
NEW = ("ipt_smooth_device", "ipt_pgm_device", "ipt_pgm", "ipt_logf_host", "ipt_logf_device")


def test_symbols_declared_bound_and_exported():
    txt = (ROOT / "include" / "ipt_capi.h").read_text()
    assert re.search(r"#define\s+IPT_ABI_VERSION\s+7\b", txt)
    assert capi.ABI_VERSION == 7
    lib = capi.load()
    assert lib.ipt_abi_version() == 7
    for sym in NEW:
        assert re.search(rf"^int {sym}\(", txt, re.M), sym
        assert sym in capi.EXPORTED_SYMBOLS
        assert hasattr(lib, sym)
    for name in ("PgmParams", "make_pgm_params", "logf_host"):
        assert hasattr(capi, name)
    for name in ("smooth_device", "pgm_device", "pgm", "logf_device"):
        assert hasattr(capi.Context, name)
    # the struct: the header's fields in the header's order, 8 x 4 bytes
    body = re.search(r"typedef struct ipt_pgm_params \{(.*?)\} ipt_pgm_params;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert fields == [f[0] for f in capi.PgmParams._fields_]
    assert C.sizeof(capi.PgmParams) == 32
    assert [getattr(capi.PgmParams, f).offset for f in fields] == list(range(0, 32, 4))
    p = capi.make_pgm_params(7, 5)
    assert (p.smooth_side, p.max_side, p.flags) == (0, 0, 0)
    assert _b(p.contrast) == _b(500.0) and _b(p.gamma) == _b(0.6)


def test_cli_smoothed_max_refusals():
    """--smoothed-max is computeSmoothedMax before the PGM: refused with the Gui
    plane and without --pgm, before any device is touched."""
    exe = ge.build_host()
    r = subprocess.run([str(exe), "--gui-plane", "--smoothed-max", "5"], capture_output=True, text=True)
    assert r.returncode == 2 and "--gui-plane" in r.stderr and "--smoothed-max" in r.stderr
    for extra in (["--smoothed-max", "5"], ["--smoothed-max", "-1", "--pgm", "x.pgm"]):
        r = subprocess.run([str(exe), *extra], capture_output=True, text=True)
        assert r.returncode == 2 and "--smoothed-max" in r.stderr, extra


def test_calls_refuse_a_null_context():
    """Without a device there is no context: every new call that takes one
    returns IPT_E_INVALID for NULL before it looks at anything else (the other
    error rules need a context: tests/test_gpu_pgm.py)."""
    lib = capi.load()
    p = capi.make_pgm_params(4, 4)
    buf = np.zeros(16, np.float32)
    g8 = np.zeros(16, np.uint8)
    assert lib.ipt_smooth_device(None, buf.ctypes.data, None, 4, 4, 2, None, None) == capi.IPT_E_INVALID
    assert lib.ipt_pgm_device(None, C.byref(p), buf.ctypes.data, None, None, g8.ctypes.data, None,
                              None) == capi.IPT_E_INVALID
    assert lib.ipt_pgm(None, C.byref(p), buf.ctypes.data, None, None, g8.ctypes.data, None) == capi.IPT_E_INVALID
    assert lib.ipt_logf_device(None, buf.ctypes.data, buf.ctypes.data, 16) == capi.IPT_E_INVALID
