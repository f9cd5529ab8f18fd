"""Display statistics on the GPU (ipt_display_stats_device / ipt_display_stats,
ipt_post.hip): the Gui's histogram, the white point by rank and the tone map
and 8-bit picture it gives, bit for bit against tests/stats_ref.py (numpy,
pinned to the reference's CImg by tests/golden/ref_display_stats.bin) on the
inputs of tests/stats_cases.py. Device buffers are torch tensors."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import display_ref as dr
import stats_cases as sc
import stats_ref as sr
from ipt_amd import capi, scenes
from test_display_cpu import read_png_gray8

pytestmark = pytest.mark.gpu

ALL = ("processed", "tone", "gray8", "hist", "stats")
HIST_SENTINEL = 0xdeadbeef


def run_stats(ctx, px, W, H, cutoff=0.0, nb=400, rank=-1, want=ALL, offset=0, stream=None, hist_len=None):
    """ipt_display_stats_device on torch tensors; the outputs not in `want` are
    passed as NULL. `offset` floats / bytes of slack in front of every image
    buffer (unaligned base pointers); `hist_len` > nb leaves a guarded tail."""
    import torch

    n = W * H
    src = torch.zeros(n + offset, dtype=torch.float32, device="cuda")
    src[offset:] = torch.from_numpy(np.array(px, np.float32).reshape(-1)).cuda()
    fb = {k: torch.full((n + offset,), -7.0, dtype=torch.float32, device="cuda") for k in ("processed", "tone")}
    g8 = torch.full((n + offset,), 9, dtype=torch.uint8, device="cuda")
    hl = max(hist_len or nb, 1) + 1
    hist = torch.from_numpy(np.full(hl, HIST_SENTINEL, np.uint32).view(np.int32)).cuda()
    stats = torch.full((5,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def ptr(t, name):
        return t.data_ptr() + offset * t.element_size() if name in want else None

    ctx.display_stats_device(capi.make_display_stats_params(W, H, cutoff, nb, rank),
                             src.data_ptr() + offset * src.element_size(),
                             ptr(fb["processed"], "processed"), ptr(fb["tone"], "tone"), ptr(g8, "gray8"),
                             hist.data_ptr() if "hist" in want else None,
                             stats.data_ptr() if "stats" in want else None, stream)
    ctx.wait()
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy()[offset:] for k, v in fb.items()}
    out["gray8"] = g8.cpu().numpy()[offset:]
    out["hist"] = hist.cpu().numpy().view(np.uint32)
    out["stats"] = stats.cpu().numpy()
    assert np.array_equal(src.cpu().numpy()[offset:].view(np.uint32), dr.bits(px).reshape(-1)), "input was written"
    for t in list(fb.values()) + [g8]:  # nothing in front of the base pointer is touched
        head = t.cpu().numpy()[:offset]
        assert (head == (9 if t.dtype == torch.uint8 else -7.0)).all()
    # what was not asked for is untouched, and nothing past the counts / the four floats is written
    for k in ("processed", "tone"):
        if k not in want:
            assert (out[k] == -7.0).all(), k
    if "gray8" not in want:
        assert (out["gray8"] == 9).all()
    used = nb if "hist" in want else 0
    assert (out["hist"][used:] == HIST_SENTINEL).all()
    out["hist"] = out["hist"][:used]
    assert out["stats"][4] == -7.0 and ("stats" in want or (out["stats"] == -7.0).all())
    out["stats"] = out["stats"][:4]
    return out


def assert_same(got, ref, keys=ALL, tag=None):
    for k in keys:
        a, b = (got[k], ref[k]) if k in ("gray8", "hist") else (dr.bits(got[k]), dr.bits(ref[k]))
        assert a.shape == b.shape, (tag, k, a.shape, b.shape)
        bad = a != b
        assert not bad.any(), (tag, k, int(bad.sum()), np.flatnonzero(bad)[:5], a[bad][:5], b[bad][:5])


# ---- 1. shapes ----------------------------------------------------------------
@pytest.mark.parametrize("glare", (False, True), ids=("plain", "glare"))
@pytest.mark.parametrize("W,H", sc.SHAPES, ids=[f"{W}x{H}" for W, H in sc.SHAPES])
def test_shapes(gpu_ctx, oracle, W, H, glare):
    img, k, ref = sc.shape_ref(W, H, glare)
    assert_same(run_stats(gpu_ctx, img, W, H, sc.CUTOFF if glare else 0.0, 400, k), ref, tag=(W, H, glare))


@pytest.mark.parametrize("glare", (False, True), ids=("plain", "glare"))
@pytest.mark.parametrize("W,H", sc.OFFSET_SHAPES, ids=[f"{W}x{H}" for W, H in sc.OFFSET_SHAPES])
def test_unaligned_base_pointers(gpu_ctx, oracle, W, H, glare):
    """Every image buffer one float (one byte for gray8) past 16-byte alignment."""
    img, k, ref = sc.shape_ref(W, H, glare)
    assert_same(run_stats(gpu_ctx, img, W, H, sc.CUTOFF if glare else 0.0, 400, k, offset=1), ref, tag=(W, H, glare))


# ---- 2. histogram edges ---------------------------------------------------------
@pytest.mark.parametrize("name,W,H,img,nb", sc.hist_edge_cases(), ids=[c[0] for c in sc.hist_edge_cases()])
def test_histogram_edges(gpu_ctx, name, W, H, img, nb):
    ref = sr.stats_ref(img, W, H, 0.0, nb, -1)
    got = run_stats(gpu_ctx, img, W, H, 0.0, nb, -1, hist_len=4096)
    assert_same(got, ref, tag=name)
    if name in ("constant", "zeros"):
        assert got["hist"][-1] == W * H
    if name == "nan_first":
        assert not got["hist"].any() and np.isnan(got["stats"][:3]).all()


def test_histogram_of_the_cimg_fixture(gpu_ctx):
    """The reference's own CImg counts, maximum and kth_smallest."""
    for c in sr.cimg_cases():
        got = run_stats(gpu_ctx, c["px"], c["W"], c["H"], 0.0, c["nb"], c["k"], want=("hist", "stats"))
        assert np.array_equal(got["hist"], c["hist"]), c["name"]
        assert sr.bits1(got["stats"][0]) == sr.bits1(c["mx"]), c["name"]
        assert sr.bits1(got["stats"][2]) == sr.bits1(c["kth"]), c["name"]


# ---- 3. selection edges ---------------------------------------------------------
@pytest.mark.parametrize("name,W,H,img,ranks", sc.select_edge_cases(), ids=[c[0] for c in sc.select_edge_cases()])
def test_selection_edges(gpu_ctx, name, W, H, img, ranks):
    for k in ranks:
        ref = sr.stats_ref(img, W, H, 0.0, 0, k)
        got = run_stats(gpu_ctx, img, W, H, 0.0, 0, k, want=("tone", "gray8", "stats"))
        assert_same(got, ref, keys=("tone", "gray8", "stats"), tag=(name, k))


def test_percentile_white_point(gpu_ctx):
    W, H, img = sc.percentile_image()
    k = sr.white_rank_for(W, H, 0.95)
    ref = sr.stats_ref(img, W, H, 0.0, 400, k)
    got = run_stats(gpu_ctx, img, W, H, 0.0, 400, k)
    assert_same(got, ref)
    assert got["stats"][2] < got["stats"][0] and (got["tone"] == 1.0).mean() >= 0.01


# ---- 4. equivalence and skipped stages -------------------------------------------
@pytest.mark.parametrize("cutoff", (0.0, sc.CUTOFF), ids=("plain", "glare"))
def test_rank_minus_one_equals_display_device(gpu_ctx, cutoff):
    from test_gpu_display import run_device

    W, H = 97, 33
    img = sc.shape_image(W, H)
    base = run_device(gpu_ctx, img, W, H, cutoff)
    got = run_stats(gpu_ctx, img, W, H, cutoff, 400, -1)
    assert_same(got, base, keys=("processed", "tone", "gray8"))
    assert sr.bits1(got["stats"][2]) == sr.bits1(got["stats"][0])


def test_null_outputs_skip_their_stages(gpu_ctx, oracle):
    W, H = 97, 33
    img = sc.shape_image(W, H)
    k = sr.white_rank_for(W, H, 0.95)
    ref = sr.stats_ref(img, W, H, sc.CUTOFF, 400, k)
    for want in (("hist",), ("stats",), ("hist", "stats"), ("tone",), ("gray8",), ("processed",),
                 ("gray8", "hist"), ("processed", "tone", "gray8")):
        nb = 400 if "hist" in want else 0
        got = run_stats(gpu_ctx, img, W, H, sc.CUTOFF, nb, k, want=want)  # (asserts the rest untouched)
        assert_same(got, ref, keys=want, tag=want)
    # hist_buckets = 0 with a buffer passed: the buffer is not written
    got = run_stats(gpu_ctx, img, W, H, sc.CUTOFF, 0, k, want=ALL, hist_len=8)
    assert_same(got, ref, keys=("processed", "tone", "gray8", "stats"))


# ---- 5. scratch and streams -----------------------------------------------------
def test_consecutive_calls_reset_the_scalars(gpu_ctx):
    rng = np.random.default_rng(71)
    a = (rng.random(64 * 48, dtype=np.float32) * np.float32(3.0)).astype(np.float32)
    b = (rng.random(64 * 48, dtype=np.float32) * np.float32(0.02)).astype(np.float32)
    for img, k in ((a, 100), (b, 3000), (a, 3000), (b, 0)):
        assert_same(run_stats(gpu_ctx, img, 64, 48, 0.0, 400, k), sr.stats_ref(img, 64, 48, 0.0, 400, k), tag=k)


def test_small_after_large_on_a_fresh_context(oracle):
    ctx = capi.Context(0)
    try:
        for W, H in ((37, 23), (640, 640), (37, 23)):
            img, k, ref = sc.shape_ref(W, H, True)
            got = run_stats(ctx, img, W, H, sc.CUTOFF, 400, k, want=("gray8", "hist", "stats"))
            assert_same(got, ref, keys=("gray8", "hist", "stats"), tag=(W, H))
    finally:
        ctx.close()


def test_two_streams_share_the_scratch():
    """Two calls on two streams of one context with no host wait between them:
    the second runs behind the first (the context's event), each with its own
    scalars, digit counts and tone scratch."""
    import torch

    ctx = capi.Context(0)
    try:
        (WL, HL), (WS, HS) = (1024, 1024), (37, 23)
        L, kL, refL = sc.shape_ref(WL, HL, False)
        S, kS, refS = sc.shape_ref(WS, HS, False)
        dev = {"L": torch.from_numpy(np.array(L)).cuda(), "S": torch.from_numpy(np.array(S)).cuda()}
        shape = {"L": (WL, HL, kL, refL), "S": (WS, HS, kS, refS)}
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()

        def buffers(key):
            W, H, _, _ = shape[key]
            return (key, torch.full((W * H,), 9, dtype=torch.uint8, device="cuda"),
                    torch.zeros(400, dtype=torch.int32, device="cuda"),
                    torch.zeros(4, dtype=torch.float32, device="cuda"))

        def queue(bufs, stream):  # queues only, no synchronisation of any kind
            key, g8, hist, st = bufs
            W, H, k, _ = shape[key]
            ctx.display_stats_device(capi.make_display_stats_params(W, H, 0.0, 400, k), dev[key].data_ptr(), None,
                                     None, g8.data_ptr(), hist.data_ptr(), st.data_ptr(), stream.cuda_stream)

        warm = buffers("L")
        torch.cuda.synchronize()
        queue(warm, s1)  # grows the scratch, so that no later call takes the allocating path
        ctx.wait()
        out = [warm]
        for first, second in (("L", "S"), ("S", "L"), ("L", "S")):
            a, b = buffers(first), buffers(second)
            torch.cuda.synchronize()
            queue(a, s1)
            queue(b, s2)
            ctx.wait()
            torch.cuda.synchronize()
            out += [a, b]
        for i, (key, g8, hist, st) in enumerate(out):
            ref = shape[key][3]
            assert np.array_equal(g8.cpu().numpy(), ref["gray8"]), (i, key)
            assert np.array_equal(hist.cpu().numpy().view(np.uint32), ref["hist"]), (i, key)
            assert np.array_equal(dr.bits(st.cpu().numpy()), dr.bits(ref["stats"])), (i, key)
    finally:
        ctx.close()


# ---- 6. end to end --------------------------------------------------------------
E2E = dict(W=64, H=64, spp=4, passes=4, n_rays=4, depth=3)


def test_render_then_stats_on_one_stream(gpu_ctx):
    """render_device_async x 4 passes into a device-resident Gui plane, then
    display_stats_device behind it on the same stream, no wait in between."""
    import torch

    W, H = E2E["W"], E2E["H"]
    gpu_ctx.upload_scene(scenes.make_scene_box())
    A = torch.zeros(4, H, W, dtype=torch.float32, device="cuda")
    g8 = torch.zeros(W * H, dtype=torch.uint8, device="cuda")
    hist = torch.zeros(400, dtype=torch.int32, device="cuda")
    st = torch.zeros(4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    k = capi.white_rank_for(W, H, 0.95)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for i in range(E2E["passes"]):
            p = capi.make_params(W, H, E2E["spp"], spp_offset=i * E2E["spp"], n_rays=E2E["n_rays"],
                                 depth_max=E2E["depth"], flags=capi.IPT_FLAG_GUI_PLANE)
            gpu_ctx.render_device_async(p, *(A[j].data_ptr() for j in range(4)), s.cuda_stream)
        gpu_ctx.display_stats_device(capi.make_display_stats_params(W, H, 0.0, 400, k), A[0].data_ptr(), None, None,
                                     g8.data_ptr(), hist.data_ptr(), st.data_ptr(), s.cuda_stream)
    s.synchronize()
    gpu_ctx.wait()
    plane = A[0].cpu().numpy().reshape(-1)
    assert plane.max() > 0
    ref = sr.stats_ref(plane, W, H, 0.0, 400, k)
    assert np.array_equal(g8.cpu().numpy(), ref["gray8"])
    assert np.array_equal(hist.cpu().numpy().view(np.uint32), ref["hist"])
    assert np.array_equal(dr.bits(st.cpu().numpy()), dr.bits(ref["stats"]))


def test_cli_white_percentile_and_histogram(tmp_path):
    exe = ge.build_host()
    W, H = E2E["W"], E2E["H"]
    subprocess.run([str(exe), "--scene", "box", "--width", str(W), "--height", str(H), "--spp", str(E2E["spp"]),
                    "--passes", str(E2E["passes"]), "--n-rays", str(E2E["n_rays"]), "--depth", str(E2E["depth"]),
                    "--gui-plane", "--gpu-display", "--white-percentile", "0.95",
                    "--histogram", str(tmp_path / "hist.txt"), "--pfm", str(tmp_path / "plane.pfm"),
                    "--out", str(tmp_path / "out.png")], check=True, capture_output=True, timeout=120)
    raw = (tmp_path / "plane.pfm").read_bytes()
    plane = np.frombuffer(raw[-4 * W * H:], "<f4").reshape(H, W)[::-1].reshape(-1)  # PFM rows run bottom to top
    ref = sr.stats_ref(plane, W, H, 0.0, 400, sr.white_rank_for(W, H, 0.95))
    assert np.array_equal(read_png_gray8(tmp_path / "out.png"), ref["gray8"])
    counts = np.array((tmp_path / "hist.txt").read_text().split(), np.uint32)
    assert np.array_equal(counts, ref["hist"])
    assert ref["stats"][2] < ref["stats"][0]


# ---- 7. host buffers and errors ---------------------------------------------------
def test_host_call_equals_device_call(gpu_ctx, oracle):
    W, H = 53, 21
    img = sc.shape_image(W, H)
    k = sr.white_rank_for(W, H, 0.95)
    for cutoff in (0.0, sc.CUTOFF):
        assert_same(gpu_ctx.display_stats(img, W, H, cutoff, 400, k), sr.stats_ref(img, W, H, cutoff, 400, k), tag=cutoff)


def test_argument_errors(gpu_ctx):
    W, H = 16, 8
    img = np.ones(W * H, np.float32)
    hist = np.full(4096, 7, np.uint32)
    lib, h = gpu_ctx.lib, gpu_ctx.h

    def rc(px=img.ctypes.data, hp=hist.ctypes.data, **kw):
        args = dict(width=W, height=H, glare_cutoff=0.0, hist_buckets=400, white_rank=-1, flags=0)
        args.update(kw)
        return lib.ipt_display_stats(h, C.byref(capi.make_display_stats_params(**args)), px, None, None, None, hp, None)

    assert rc() == capi.IPT_OK and hist[:400].sum() == W * H and (hist[400:] == 7).all()
    hist[:] = 7
    assert rc(hist_buckets=-1) == capi.IPT_E_INVALID
    assert rc(hist_buckets=4097) == capi.IPT_E_INVALID
    assert rc(hist_buckets=4096) == capi.IPT_OK
    hist[:] = 7
    assert rc(hp=None) == capi.IPT_E_INVALID
    assert rc(hp=None, hist_buckets=0) == capi.IPT_OK
    assert rc(flags=1) == capi.IPT_E_UNSUPPORTED
    assert rc(px=None) == capi.IPT_E_INVALID
    assert rc(width=0) == capi.IPT_E_INVALID
    assert rc(height=-1) == capi.IPT_E_INVALID
    assert rc(glare_cutoff=-1.0) == capi.IPT_E_INVALID
    assert rc(glare_cutoff=float("nan")) == capi.IPT_E_INVALID
    assert rc(glare_cutoff=float("inf")) == capi.IPT_E_UNSUPPORTED
    assert lib.ipt_display_stats(h, None, img.ctypes.data, None, None, None, hist.ctypes.data, None) == capi.IPT_E_INVALID
    wide = np.zeros(4097, np.float32)
    assert rc(px=wide.ctypes.data, width=4097, height=1, glare_cutoff=1.01) == capi.IPT_E_UNSUPPORTED
    assert rc(px=wide.ctypes.data, width=4097, height=1) == capi.IPT_OK
    hist[:] = 7
    # the device call validates the same way, before a buffer is touched
    dp = capi.make_display_stats_params(W, H, 0.0, 4097, -1)
    assert lib.ipt_display_stats_device(h, C.byref(dp), 1, None, None, None, 1, None, None) == capi.IPT_E_INVALID
    assert (hist == 7).all()
    with pytest.raises(capi.IptError) as e:
        gpu_ctx.display_stats(img, W, H, 0.0, 5000, -1)
    assert e.value.code == capi.IPT_E_INVALID
