"""The Gui render plane's restatement (tests/gui_cases.py) and the host side of
IPT_FLAG_GUI_PLANE, without a GPU.

tests/test_gpu_gui_plane.py compares the kernels with gui_cases bit for bit;
that is worth what the restatement is worth. Here it is tied to what is
pinned to compiled reference code -- the oracle's GridRenderPlane codes and
replay -- through the Grid-row-plus-one identity, its edge samples are
confirmed with the oracle's randf, its histograms are pinned, the C++
GuiRenderPlane::addRay is held against it, two wrong replays are shown to
differ on the frames the GPU tests use, and ipt_shard_plan's Gui candidates
are checked against every sample's actual destination."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import drift_cases as dc
import gui_cases as gc
import oracle_binding as ob
from ipt_amd import capi, scenes, tiles

bits = dc.bits
HERE = Path(__file__).resolve().parent
SEED = dc.DEFAULT_SEED

# every frame of the edge table at passes 0..1, and the renders with edge samples
IDENTITY = tuple(f + (2, 0) for f in gc.TABLE_FRAMES if f != gc.SQUARE) + gc.EDGE_RENDERS


def _id(k):
    return "%dx%dx%d@%d" % k


@pytest.mark.parametrize("key", IDENTITY, ids=_id)
def test_gui_row_is_grid_row_plus_one(oracle, key):
    """Away from source rows 0 and H-1: Gui row == Grid row + 1 and equal
    codes, the Grid side being the oracle's. On the two edge rows the codes
    differ exactly at the top clamps (Gui 0x5, Grid dy = +1) and the bottom
    samples (Gui dy = +1, Grid dy = 0)."""
    W, H, spp, off = key
    _, oc, _ = dc.oracle_samples(W, H, spp, off)
    assert np.array_equal(gc.grid_codes(W, H, spp, off), oc)  # the stream and the jitter, restated
    c = gc.codes(W, H, spp, off)
    _, gy, gx = gc.destinations(c)
    _, oy, ox = dc.destinations(oc)
    inner = slice(1, H - 1)
    assert np.array_equal(gy[:, inner], oy[:, inner] + 1) and np.array_equal(gx[:, inner], ox[:, inner])
    assert np.array_equal(c[:, inner], oc[:, inner])
    top, bottom = gc.edge_masks(W, H, spp, off)
    assert np.array_equal(c != oc, top | bottom)
    assert (c[top] == 0x05).all() and (((oc[top] >> 2) & 3) == 2).all() and (gy[top] == H - 1).all()
    assert (((c[bottom] >> 2) & 3) == 2).all() and (((oc[bottom] >> 2) & 3) == 1).all() and (gy[bottom] == 1).all()
    assert not (c >= 0x10).any()


@pytest.mark.parametrize("key", sorted(gc.HIST), ids=_id)
def test_gui_histograms_pinned(oracle, key):
    W, H, spp, off = key
    assert dc.histogram(gc.codes(W, H, spp, off)) == gc.HIST[key]
    if off == 0 and (W, H, spp) in dc.HIST and spp == 2:
        assert gc.HIST[key] == dc.HIST[W, H, spp]  # no edge sample in passes 0..1: the Grid's figures


def test_wide_frame_at_nine_passes_has_no_dy_plus_one():
    assert 0x9 in dc.HIST[60000, 3, 9] and 0x9 not in gc.HIST[60000, 3, 9, 0]
    top, bottom = gc.edge_masks(60000, 3, 9)
    assert [tuple(i) for i in np.argwhere(top)] == [(7, 0, 2420), (8, 0, 17598)] and not bottom.any()


def test_tallest_frame_passes_136_to_144_hold_both_edges():
    W, H = dc.MAX_HEIGHT
    top, bottom = gc.edge_masks(W, H, 9, 136)
    assert [tuple(i) for i in np.argwhere(top)] == [(143 - 136, 0, 1)]
    assert [tuple(i) for i in np.argwhere(bottom)] == [(0, H - 1, 1), (143 - 136, H - 1, 1)]
    c = gc.codes(W, H, 9, 136)
    assert (c[bottom] == 0x09).all()


@pytest.mark.parametrize("frame", gc.TABLE_FRAMES, ids=lambda f: "%dx%d" % f)
def test_edge_samples(oracle, frame):
    """The edge table: a scan of source rows 0 and H-1 finds exactly the
    listed samples, and each is confirmed draw by draw with the oracle's
    randf (draw 1 of the path is the y jitter)."""
    W, H = frame
    top, bottom = gc.edge_scan(W, H, gc.SCAN_PASSES[frame])
    assert top == gc.TOP_CLAMP[frame] and bottom == gc.BOTTOM[frame]
    for samples, row, want in ((top, 0, H), (bottom, H - 1, 1)):
        for s, ix in samples:
            u1 = np.float32(oracle.ipt_oracle_randf(SEED, s, row * W + ix, 1))
            y = (np.float32(row) + u1) / np.float32(H)
            assert int(np.float32(H) - y * np.float32(H)) == want
            if row == 0:  # y*H below half an ulp of H: within 2^-24 of the view's edge
                assert y <= np.float32(2.0 ** -24)


def test_each_edge_kind_has_a_nonzero_sample(oracle):
    """Across the GPU suite's renders: a bottom sample with radiance in the box
    scene (640^2, pass 56) and a top clamp with radiance (pass 143 in
    smallpt's room; in the box scene no ray at the view's lower edge carries any, so every
    listed top clamp is zero there: it still shows in counters and means)."""
    v, _, _ = dc.oracle_samples(640, 640, 1, 56)
    _, bottom = gc.edge_masks(640, 640, 1, 56)
    assert bottom.sum() == 1 and (v[bottom] > 0).all()
    for W, H, spp, off in gc.EDGE_RENDERS:
        top, _ = gc.edge_masks(W, H, spp, off)
        assert not (dc.oracle_samples(W, H, spp, off)[0][top] > 0).any()
    name, W, H, spp, off = gc.TOP_CLAMP_NONZERO
    p = capi.make_params(W, H, spp, spp_offset=off, n_rays=dc.N_RAYS, depth_max=dc.DEPTH_MAX)
    v, _ = ob.render_values(getattr(scenes, "make_scene_" + name)(), p)
    top, _ = gc.edge_masks(W, H, spp, off)
    assert top.sum() == 1 and (v[top] > 0).all()


# ---- the C++ GuiRenderPlane -------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    ge.build_lib()
    ge.build_host()
    exe = tmp_path_factory.mktemp("gui") / "gui_plane_probe"
    subprocess.run(["g++", *ge.GXX_FLAGS, "-o", str(exe), str(HERE / "native" / "gui_plane_probe.cpp"),
                    f"-I{ge.HOST}", f"-L{ge.LIB.parent}", "-lipt_host", "-lipt_hip",
                    f"-Wl,-rpath,{ge.LIB.parent}", "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    return exe


@pytest.mark.parametrize("key", [(640, 640, 1, 25), (640, 640, 1, 56), (2, 65536, 9, 136), (13, 11, 9, 0)], ids=_id)
def test_cpp_addray_is_the_restatement(oracle, probe, tmp_path, key):
    """GuiRenderPlane::addRay over whole passes in raster order (both edge
    kinds among them) gives the restated plane's pixels and counters."""
    W, H, spp, off = key
    v, _, _ = dc.oracle_samples(W, H, spp, off)
    x, y = gc.coords(W, H, spp, off)
    np.stack([x, y, v], axis=-1).astype(np.float32).tofile(tmp_path / "in.xyv")
    subprocess.run([str(probe), "addray", str(W), str(H), str(tmp_path / "in.xyv"), str(tmp_path / "out.bin")],
                   check=True)
    raw = np.fromfile(tmp_path / "out.bin", np.uint32)
    ref = gc.gui_plane(W, H, spp, off)
    assert np.array_equal(raw[:W * H], bits(ref["pixels"]))
    assert np.array_equal(raw[W * H:], ref["counters"])


def test_cpp_reset_image(probe):
    out = subprocess.run([str(probe), "reset", "7", "5"], check=True, capture_output=True, text=True).stdout
    assert int(out) == 0


@pytest.mark.parametrize("extra", [["--smooth", "3"], ["--pgm", "x.pgm"]])
def test_cli_refuses_grid_only_outputs_with_the_gui_plane(extra):
    """--smooth is GridRenderPlane::smooth and --pgm main.cpp's writer for it:
    refused with a message before any device is touched."""
    exe = ge.build_host()
    r = subprocess.run([str(exe), "--gui-plane", *extra], capture_output=True, text=True)
    assert r.returncode == 2 and "--gui-plane" in r.stderr and extra[0] in r.stderr


# ---- the replay ---------------------------------------------------------------
def test_numpy_replay_continues_a_preloaded_plane_as_the_oracle(oracle):
    """drift_cases._add_rays on existing state (the preloaded kinds) is
    ob.accumulate's addRay: under the Grid codes the two agree bit for bit, so
    the Gui replay into a preloaded plane differs from the pinned one by its
    destinations alone."""
    W, H, spp = 60000, 3, 9
    v, oc, _ = dc.oracle_samples(W, H, spp)
    _, yi, xi = dc.destinations(oc)
    d = oc != 0x05
    pre, _ = dc.preload(W, H, spp, yi[d] * W + xi[d])
    ref = ob.accumulate(v, oc, img=dc.copy_plane(pre))
    got = gc.replay_events(v, yi, xi, img=dc.copy_plane(pre))
    for k in ref:
        assert np.array_equal(bits(got[k]), bits(ref[k])), k


@pytest.mark.parametrize("key", gc.EDGE_RENDERS, ids=_id)
def test_wrong_replays_differ(oracle, key):
    """Without the min() (a top clamp falls off the image, row H) and with the
    Grid's doubled row 0 kept, the plane is another one -- on the frames the
    GPU tests render. (A frame without a top clamp is the same without the
    min: 640^2 at pass 56.)"""
    W, H, spp, off = key
    v, _, _ = dc.oracle_samples(W, H, spp, off)
    ref = gc.gui_plane(W, H, spp, off)
    top, _ = gc.edge_masks(W, H, spp, off)
    no_clamp = gc.wrong_replay(v, W, H, spp, off, "no_clamp")
    assert bool((no_clamp["counters"] != ref["counters"]).any()) == bool(top.any())
    doubled = gc.wrong_replay(v, W, H, spp, off, "grid_row0")
    assert (doubled["counters"] != ref["counters"]).any()
    assert (bits(doubled["pixels"]) != bits(ref["pixels"])).any()
    # and the Grid plane itself is another plane
    grid = dc.oracle_plane(W, H, spp, off)
    assert (bits(grid["pixels"]) != bits(ref["pixels"])).any()


def test_wrong_replay_without_clamp_changes_pixels_where_it_has_radiance(oracle):
    name, W, H, spp, off = gc.TOP_CLAMP_NONZERO
    p = capi.make_params(W, H, spp, spp_offset=off, n_rays=dc.N_RAYS, depth_max=dc.DEPTH_MAX)
    v, _ = ob.render_values(getattr(scenes, "make_scene_" + name)(), p)
    ref = gc.replay(v, gc.codes(W, H, spp, off))
    bad = gc.wrong_replay(v, W, H, spp, off, "no_clamp")
    assert (bits(bad["pixels"]) != bits(ref["pixels"])).any()


# ---- ipt_shard_plan -----------------------------------------------------------
PLANS = ((1, 2), (1, 3), (7, 3), (16, 8))


@pytest.mark.parametrize("tile,n_shards", PLANS)
@pytest.mark.parametrize("frame", [dc.TALL, dc.SMALL], ids=lambda f: "%dx%d" % f)
def test_shard_plan_follows_the_gui_map(frame, tile, n_shards):
    """With the flag: the same owned rows; every sample's actual destination
    row has its source row among the owner's candidates; the candidates are
    the nominal sources +-1 under the Gui map, not the Grid plan's.

    Two of the plans cannot differ between the maps: with one-row tiles dealt
    to two shards every row is within one of an owned row, so each shard's
    candidates are all rows under either map, and 16-row tiles on the 11-row
    frame are a single tile. There the plans are asserted equal."""
    W, H = frame
    _, yi, _ = gc.destinations(gc.codes(W, H, 2))
    src = np.broadcast_to(np.arange(H)[None, :, None], yi.shape)
    differs = False
    for s in range(n_shards):
        kw = dict(tile_rows=tile, n_shards=n_shards, shard_id=s)
        owned, cand = capi.shard_plan(capi.make_params(W, H, 1, flags=gc.FLAG, **kw))
        g_owned, g_cand = capi.shard_plan(capi.make_params(W, H, 1, **kw))
        assert np.array_equal(owned, g_owned)
        assert np.array_equal(owned, dc.shard_of(np.arange(H), tile, n_shards) == s)
        mine = owned[yi]
        assert np.isin(src[mine], cand).all()
        want = np.zeros(H, bool)
        for dy in (-1, 0, 1):
            y = H - 1 - np.arange(H) + dy
            ok = (y >= 0) & (y < H)
            want[ok] |= owned[y[ok]]
        assert np.array_equal(cand, np.flatnonzero(want))
        differs |= not np.array_equal(cand, g_cand)
    assert differs == (not ((tile, n_shards) == (1, 2) or tile >= H))
    rows = tiles.owned_rows(W, H, tile, n_shards, flags=gc.FLAG)
    assert all(np.array_equal(a, b) for a, b in zip(rows, tiles.owned_rows(W, H, tile, n_shards)))


def test_abi_version_and_flag():
    assert capi.ABI_VERSION == 7 and capi.IPT_FLAG_GUI_PLANE == 2
    assert capi.load().ipt_abi_version() == 7
    hdr = (HERE.parent / "include" / "ipt_capi.h").read_text()
    assert "#define IPT_ABI_VERSION 7" in hdr and "IPT_FLAG_GUI_PLANE = 2u" in hdr
