"""Host check of the box planes' nearest-candidate form
(ipt_path.h trace_box_planes_nearest): bit-identical t and
prim to trace_box_planes_only, and the returned hit point bit-identical to
o + d*t, on 20 M rays per INRANGE form (tests/native/box_planes_check.cpp lists
the ray classes). Every outcome class of the new form -- no candidate, the
candidate hits, monotone miss, the full form -- must occur. The GPU half is
tests/test_gpu_box_planes.py."""
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = tmp_path_factory.mktemp("boxplanes") / "box_planes_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-DIPT_HD=inline", "-o", str(exe),
                    str(HERE / "native" / "box_planes_check.cpp")], check=True)
    r = subprocess.run([str(exe), "20000000"], capture_output=True, text=True)
    rows = dict()
    for line in r.stdout.split("\n"):
        w = line.split()
        if w and w[0] == "inrange":
            rows[int(w[1])] = {w[i]: int(w[i + 1]) for i in range(2, len(w) - 1, 2)}
    print(r.stdout)
    return r.returncode, rows, r.stdout


@pytest.mark.parametrize("inrange", [0, 1])
def test_nearest_form_matches_full_form(report, inrange):
    rc, rows, out = report
    assert inrange in rows, out
    row = rows[inrange]
    assert row["rays"] >= 20_000_000
    assert row["mismatches"] == 0, out
    for cls in ("none", "hit", "mono", "full", "sphere_hits"):
        assert row[cls] > 0, (cls, out)
    assert rc == 0, out
