"""Display pipeline, CPU side: ipt_math.h's powf_ (the library's host build,
ipt_powf_host) against the host libm powf bit for bit, and the tests' CPU
reference of the pipeline (tests/display_ref.py) against the host path the
project already ships (ipt_host.cpp tone_map / to_gray8 through
tests/native/host_scene_dump.cpp). Also the conditions under which the
large-shape and denormal inputs of tests/display_cases.py discriminate, which
the GPU tests rely on."""
import os
import struct
import subprocess
import zlib
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import display_cases as dc
import display_ref as dr
from ipt_amd import capi

HERE = Path(__file__).resolve().parent
ONE = 0x3f800000
P = float(dr.GAMMA)       # Gui's 1/2.2
PGM_GAMMA = 0.6           # main.cpp's PGM gamma


def _patterns(lo, hi, stride):
    return np.arange(lo, hi, stride, dtype=np.uint64).astype(np.uint32).view(np.float32)


def _assert_bits(x, y):
    a, b = dr.bits(capi.powf_host(x, y)), dr.bits(dr.libm_powf(x, y))
    bad = a != b
    assert not bad.any(), (y, dr.bits(x)[bad][:5], a[bad][:5], b[bad][:5])


def _sweep_unit(y, stride):
    chunk = (1 << 24) * stride
    for s in range(0, ONE + 1, chunk):
        _assert_bits(_patterns(s, min(ONE + 1, s + chunk), stride), y)


def test_powf_unit_interval_strided():
    """Every 61st float of [0, 1] plus both ends, y = 1/2.2."""
    _sweep_unit(P, 61)
    _assert_bits(np.array([0, 1, 0x007fffff, 0x00800000, ONE - 1, ONE], np.uint32).view(np.float32), P)


def test_powf_unit_interval_exhaustive():
    """Every float of [0, 1], subnormals and +0 included, y = 1/2.2
    (1.07e9 evaluations on each side; 14 s on 8 threads, so not marked slow)."""
    _sweep_unit(P, 1)


def test_powf_special_and_outside():
    """-0, +inf and NaN bit for bit; the other floats (negative, above 1),
    every 4093rd pattern, after the cut to [0, 1]."""
    _assert_bits(np.array([0x80000000, 0x7f800000, 0x7fc00000, 0x7f800001, 0xffc01234], np.uint32).view(np.float32), P)
    x = _patterns(ONE + 1, 1 << 32, 4093)
    a, b = dr.cut01(capi.powf_host(x, P)), dr.cut01(dr.libm_powf(x, P))
    bad = dr.bits(a) != dr.bits(b)
    assert not bad.any(), (dr.bits(x)[bad][:5], dr.bits(a)[bad][:5], dr.bits(b)[bad][:5])


def test_powf_pgm_gamma():
    """y = 0.6f (main.cpp's PGM gamma): [0, 1] sampled every 4093rd pattern
    bit for bit, the rest after the cut."""
    _assert_bits(_patterns(0, ONE + 1, 4093), PGM_GAMMA)
    _assert_bits(np.array([ONE, 0x80000000], np.uint32).view(np.float32), PGM_GAMMA)
    x = _patterns(ONE + 1, 1 << 32, 4093)
    a, b = dr.cut01(capi.powf_host(x, PGM_GAMMA)), dr.cut01(dr.libm_powf(x, PGM_GAMMA))
    assert np.array_equal(dr.bits(a), dr.bits(b))


def test_powf_rejects_unsupported_exponents():
    x = np.ones(4, np.float32)
    for y in (0.0, -0.5, 2.0, float("inf"), float("nan")):
        with pytest.raises(capi.IptError) as e:
            capi.powf_host(x, y)
        assert e.value.code == capi.IPT_E_UNSUPPORTED


# ---- display_ref against ipt_host.cpp's to_gray8 ---------------------------
@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    ge.build_lib()
    ge.build_host()
    exe = tmp_path_factory.mktemp("host") / "host_scene_dump"
    subprocess.run(["g++", *ge.GXX_FLAGS, "-o", str(exe), str(HERE / "native" / "host_scene_dump.cpp"),
                    f"-I{ge.HOST}", f"-L{ge.LIB.parent}", "-lipt_host", "-lipt_hip",
                    f"-Wl,-rpath,{ge.LIB.parent}", "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    return exe


def read_png_gray8(path):
    data = Path(path).read_bytes()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, {}
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        typ, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(typ + body)
        chunks[typ] = chunks.get(typ, b"") + body
        pos += 12 + n
    w, h, depth, ctype = struct.unpack(">IIBB", chunks[b"IHDR"][:10])
    assert (depth, ctype) == (8, 0)
    raw = np.frombuffer(zlib.decompress(chunks[b"IDAT"]), np.uint8).reshape(h, w + 1)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(-1)


def _images():
    rng = np.random.default_rng(21)
    W, H = 37, 23
    rnd = (rng.random(W * H, dtype=np.float32) * np.float32(3.0)).astype(np.float32)
    rnd[5] = 0.0
    one_nan = rnd.copy()
    one_nan[100] = np.nan
    return [("random", W, H, rnd), ("constant", 9, 5, np.full(45, 0.75, np.float32)),
            ("one_nan", W, H, one_nan), ("1x1", 1, 1, np.array([2.5], np.float32))]


@pytest.mark.parametrize("name,W,H,px", _images(), ids=[c[0] for c in _images()])
def test_display_ref_matches_host_to_gray8(dump, tmp_path, name, W, H, px):
    px.tofile(tmp_path / "p.f32")
    subprocess.run([str(dump), "gray8", str(W), str(H), str(tmp_path / "p.f32"), str(tmp_path / "o.png")], check=True)
    got = read_png_gray8(tmp_path / "o.png")
    ref = dr.display_ref(px, W, H)
    assert np.array_equal(got, ref["gray8"]), int((got != ref["gray8"]).sum())
    if name == "constant":
        assert not ref["gray8"].any()
    if name == "one_nan":
        assert np.isnan(ref["tone"][100]) and ref["gray8"][100] == 0 and ref["gray8"].max() == 255


def test_display_ref_folds():
    """The sequential folds: NaN if and only if element 0 is NaN, otherwise the
    first occurrence of the extreme non-NaN value (the sign of a zero maximum)."""
    nan = np.float32(np.nan)
    assert np.isnan(dr.fold_max(np.array([nan, 3, 1], np.float32)))
    assert dr.fold_max(np.array([1, nan, 3], np.float32)) == 3 and dr.fold_min(np.array([1, nan, 3], np.float32)) == 1
    z = dr.fold_max(np.array([-1, -0.0, 0.0], np.float32))
    assert z == 0 and np.signbit(z)


# ---- the GPU tests' inputs discriminate (tests/display_cases.py) ------------
def test_scan_geometry_of_the_shapes():
    """The four compaction shapes reach the scan's branches they are named for."""
    geo = {(W, H): dc.scan_geometry(W * H) for W, H in dc.SCAN_SHAPES}
    assert geo[(512, 512)] == (256, 1, 256)   # every scan thread used, the last case before the loop
    assert geo[(257, 1024)] == (257, 2, 129)  # thread 128 owns one block, threads >= 129 none
    assert geo[(4096, 65)] == (260, 2, 130)
    assert geo[(640, 640)] == (400, 2, 200)
    assert dc.scan_geometry(dc.FAR_W * dc.FAR_H)[:2] == (2048, 8)
    for W, H in dc.SCAN_SHAPES:
        n = W * H
        nblk, per, used = geo[(W, H)]
        pos = dc.scan_positions(n)
        assert pos[0] == 0 and pos[-1] == n - 1 and len(pos) <= 40
        owners = {p // dc.SPAN // per for p in pos}  # scan threads that own a placed pixel
        assert {0, 1, used // 2, used // 2 + 1, used - 1} <= owners


@pytest.mark.parametrize("W,H", dc.SCAN_SHAPES, ids=[f"{W}x{H}" for W, H in dc.SCAN_SHAPES])
def test_scan_cases_are_unsaturated(oracle, W, H):
    """300 distinct bright values at the placed positions, and more than half
    of the reference's processed image below the cutoff (asserted in scan_ref)."""
    ref = dc.scan_ref(W, H)
    img, pos = dc.scan_case(W, H)
    assert np.array_equal(np.flatnonzero(img > dc.SCAN_CUTOFF), pos)
    assert ref["gray8"].max() == 255 and len(np.unique(ref["gray8"])) > 100


@pytest.mark.parametrize("cx,cy", dc.FAR_CORNERS, ids=["top_left", "bottom_right"])
def test_far_halo_image_discriminates(oracle, cx, cy):
    """4096 x 512 zeros with one bright corner: the halo with r = sqrtf((float)s)
    and with r = (float)sqrt((double)s) differ in at least 500 pixels, all of
    them at s >= 2^24, and the second is the oracle's (float)hypot."""
    s, near, far = dc.far_models(cx, cy)
    diff = dr.bits(near) != dr.bits(far)
    assert int((s >= 1 << 24).sum()) > 5000
    assert int(diff.sum()) >= 500 and not diff[s < 1 << 24].any()
    ref = dr.oracle_glare(dc.far_image(cx, cy), dc.FAR_W, dc.FAR_H, dc.FAR_CUTOFF)
    assert np.array_equal(dr.bits(far), dr.bits(ref))
    assert np.array_equal(dr.bits(dc.far_ref(cx, cy)["processed"]), dr.bits(ref))


@pytest.mark.parametrize("name,W,H,img", dc.denormal_tone_cases(), ids=[c[0] for c in dc.denormal_tone_cases()])
def test_denormal_tone_cases_are_non_trivial(name, W, H, img):
    assert img.size == W * H
    dc.check_denormal_tone_case(name, img, dr.display_ref(img, W, H))


def test_stream_cases_are_unsaturated(oracle):
    for key in ("L", "S"):
        assert dc.stream_ref(key)["gray8"].max() == 255
