"""Host check of what the path kernel's leaf elision relies on (DESIGN.md 4.15,
tests/native/leaf_elide_check.cpp): replayed through the oracle with its
iteration hook, every depth-K node (n_rays 16: K = 4, one iteration) strictly
behind the lights' plane consumes exactly three draws or one, traces no ray
that hits a light, and is worth +0 by bits -- on 65 536 paths of
sample_scenes[0] and of the 25-light lattice scene. The GPU half is
tests/test_gpu_leaf_elide.py."""
import subprocess
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import __graft_entry__ as ge  # noqa: E402

SCENES = ("box", "box_lights:5")


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    exe = tmp_path_factory.mktemp("leafelide") / "leaf_elide_check"
    subprocess.run(["g++", *ge.GXX_FLAGS, "-o", str(exe), str(HERE / "native" / "leaf_elide_check.cpp"),
                    f"-I{ge.ROOT / 'include'}", f"-I{ge.HOST}", f"-L{ge.LIB.parent}", "-lipt_host", "-lipt_hip",
                    f"-Wl,-rpath,{ge.LIB.parent}", "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    # both scenes at once: 128 x 128 pixels, 4 passes each
    procs = {s: subprocess.Popen([str(exe), s, "128", "4"], stdout=subprocess.PIPE, text=True) for s in SCENES}
    out = {}
    for s, p in procs.items():
        text = p.communicate()[0]
        w = text.split()
        row = {w[i]: int(w[i + 1]) for i in range(2, len(w) - 1, 2)} if w[:1] == ["scene"] else {}
        out[s] = (p.returncode, row, text)
        print(text)
    return out


@pytest.mark.parametrize("scene", SCENES)
def test_leaf_behind_the_plane_is_worth_plus_zero(reports, scene):
    rc, row, text = reports[scene]
    assert row, text
    assert row["paths"] >= 65536
    assert row["leaves"] > row["back"] > 0, text
    # three draws or one, and nothing else
    assert row["bad_draws"] == 0 and row["draws3"] + row["draws1"] == row["back"], text
    assert row["light_hits"] == 0, text
    assert row["nonzero"] == 0, text
    # both ways to +0 occur: the skipped light pick and the cosine pick's 0/0 behind fin_s
    assert row["skips"] > 0 and row["nan_rays"] > 0, text
    assert rc == 0, text
