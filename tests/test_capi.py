"""The C-ABI library loads and exports every symbol include/ipt_capi.h
declares; without a GPU it refuses to render (no CPU fallback)."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from ipt_amd import capi

ROOT = Path(__file__).resolve().parents[1]


def declared_symbols():
    txt = (ROOT / "include" / "ipt_capi.h").read_text()
    return sorted(set(re.findall(r"^\s*(?:const char\*|int|void)\s+(ipt_\w+)\s*\(", txt, re.M)))


def test_header_declares_expected():
    assert set(declared_symbols()) == set(capi.EXPORTED_SYMBOLS)


def test_library_exports_every_declared_symbol():
    out = subprocess.run(["nm", "-D", "--defined-only", str(capi.LIB_PATH)], check=True,
                         capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    missing = [s for s in declared_symbols() if s not in exported]
    assert not missing, missing
    lib = capi.load()
    for s in declared_symbols():
        assert hasattr(lib, s)
    assert lib.ipt_abi_version() == capi.ABI_VERSION


def test_no_cpu_fallback():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(capi.IptError) as e:
        capi.Context(0)
    assert e.value.code == capi.IPT_E_DEVICE


def test_shard_plan_partitions_rows():
    H = 100
    owners = np.zeros(H, int)
    for n_shards in (1, 2, 3, 8):
        owners[:] = 0
        for s in range(n_shards):
            p = capi.make_params(64, H, 1, tile_rows=16 if n_shards > 1 else 0,
                                 n_shards=n_shards, shard_id=s)
            owned, cand = capi.shard_plan(p)
            owners += owned
            # every source whose nominal (+-1) destination is owned is a candidate
            for iy in range(H):
                yn = max(H - 2 - iy, 0)
                if any(0 <= y < H and owned[y] for y in (yn - 1, yn, yn + 1)):
                    assert iy in cand
            assert list(cand) == sorted(cand)
        assert (owners == 1).all(), n_shards


def test_product_build_keeps_uniform_regions_structurized():
    """Round 6: with -mllvm -structurizecfg-skip-uniform-regions (rounds 4-5)
    the compiler built IPT_FLAG_COUNTERS instances that rendered different
    trees from the same source as the product instances (a code motion of the
    frame fallback; gpurun_out/diverge.log: 10 of 2048 box samples, samples
    whose camera ray misses everything given non-zero values), and the same
    source without the option is bit-exact in both. The
    product library, the A/B and the diagnostic builds leave it out."""
    import __graft_entry__ as ge
    from pathlib import Path
    assert not any("structurizecfg" in f for f in ge.HIPCC_FLAGS)
    root = Path(ge.__file__).resolve().parent
    for sh in ("variants.sh", "variants_full.sh", "regs.sh", "prof_phases.sh"):
        assert "structurizecfg" not in (root / "scripts" / sh).read_text(), sh


def test_knobs_guard_names_every_parameter():
    """ipt_knobs.h refuses an overridden parameter unless the build defines
    IPT_AB_BUILD. The guard is a hand-written list: a parameter defined under
    #ifndef but missing from it could be overridden by a stray -D without a
    word, and a name left in it after its parameter is gone guards nothing.
    The two sets are the same."""
    import re
    import __graft_entry__ as ge
    from pathlib import Path
    txt = (Path(ge.__file__).resolve().parent / "ipt_amd" / "csrc" / "ipt_knobs.h").read_text()
    defined = re.findall(r"^#ifndef\s+(IPT_\w+)\s*\n#define\s+(IPT_\w+)", txt, re.M)
    assert defined and all(a == b for a, b in defined)
    assert len(defined) == len(re.findall(r"^#ifndef\s", txt, re.M))
    guard = re.search(r"#if !defined\(IPT_AB_BUILD\)(.*?)\n#error", txt.replace("\\\n", " "), re.S)
    assert guard
    guarded = re.findall(r"defined\((IPT_\w+)\)", guard.group(1))
    assert len(guarded) == len(set(guarded))
    assert set(guarded) == {a for a, _ in defined}
