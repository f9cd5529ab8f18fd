"""Unit compaction through the C++ host layer: ipt_render --compact
(RenderParams::compact over IPT_FLAG_COMPACT) writes byte for byte the files of
the same command line without it, with and without --adaptive."""
import subprocess

import pytest

import __graft_entry__ as ge
import adaptive_cases as ac
import drift_cases as dc

pytestmark = pytest.mark.gpu

FILES = ("r.pfm", "r.u32")


def _run(tmp_path, name, extra):
    d = tmp_path / name
    d.mkdir()
    W, H = ac.LOOP_FRAMES[0]
    cmd = [str(ge.HOST_BIN), "--scene", "box", "--width", str(W), "--height", str(H), "--spp", str(ac.LOOP_SPP),
           "--n-rays", str(dc.N_RAYS), "--depth", str(dc.DEPTH_MAX), "--out", "", "--pfm", str(d / "r.pfm"),
           "--counts", str(d / "r.u32")] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return [(d / f).read_bytes() for f in FILES]


@pytest.mark.parametrize("mode", ("plain", "adaptive", "adaptive-gui"))
def test_cli_compact_writes_the_same_bytes(gpu_ctx, tmp_path, mode):
    ge.build_host()
    a = ac.LOOP_ADAPT
    extra = []
    if mode != "plain":
        extra = ["--adaptive", repr(a["rel_tol"]), "--adaptive-abs", repr(a["abs_tol"]), "--min-spp", str(a["min_count"]),
                 "--round-spp", str(ac.LOOP_ROUND)]
    if mode == "adaptive-gui":
        extra.append("--gui-plane")
    plain = _run(tmp_path, "plain", extra)
    compact = _run(tmp_path, "compact", extra + ["--compact"])
    for f, x, y in zip(FILES, plain, compact):
        assert len(x) > 0 and x == y, f
