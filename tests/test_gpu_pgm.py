"""PGM path on the GPU (ipt_smooth_device / ipt_pgm_device / ipt_pgm /
ipt_logf_device, ipt_post.hip): main.cpp's smooth -> smoothed max -> n_val on
device buffers, bit for bit against the CPU reference of tests/pgm_ref.py
(numpy float32 in the reference's order, host libm logf / powf; pinned to the
compiled reference and host layer by tests/test_pgm_cpu.py). Device buffers
are torch tensors; every comparison is on bit patterns."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import display_ref as dr
import pgm_ref as pr
from ipt_amd import capi, scenes

pytestmark = pytest.mark.gpu

EXHAUSTIVE = os.environ.get("IPT_EXHAUSTIVE") == "1"
CHUNK = 1 << 24
FILL_F, FILL_B = -7.0, 9


def _dev(a, offset=0):
    """A device copy of `a` with `offset` elements of slack in front."""
    import torch

    a = np.ascontiguousarray(a)
    t = torch.full((a.size + offset,), FILL_F if a.dtype == np.float32 else FILL_B,
                   dtype=torch.float32 if a.dtype == np.float32 else torch.uint8, device="cuda")
    t[offset:] = torch.from_numpy(a.reshape(-1).copy()).cuda()
    return t


def _ptr(t, offset=0):
    return None if t is None else t.data_ptr() + offset * t.element_size()


def _same_f(got, ref, tag):
    a, b = dr.bits(got), dr.bits(ref)
    bad = a != b
    assert not bad.any(), (tag, int(bad.sum()), np.flatnonzero(bad)[:5], a[bad][:5], b[bad][:5])


def _same_b(got, ref, tag):
    bad = got != ref
    assert not bad.any(), (tag, int(bad.sum()), np.flatnonzero(bad)[:5], got[bad][:5], ref[bad][:5])


def run_pgm(ctx, px, W, H, smooth_side=0, max_side=0, contrast=500.0, gamma=0.6, max_value=0.0, pixel_max=None,
            offset=0, stream=None, want=("smoothed", "gray8", "stats")):
    """ipt_pgm_device on torch tensors; `offset` elements of slack in front of
    every buffer. Returns the outputs asked for; checks that the inputs and
    the slack are untouched."""
    import torch

    n = W * H
    src = _dev(np.asarray(px, np.float32), offset)
    pm = None if pixel_max is None else _dev(np.asarray(pixel_max, np.float32), offset)
    bufs = {}
    if "smoothed" in want:
        bufs["smoothed"] = _dev(np.full(n, FILL_F, np.float32), offset)
    if "gray8" in want:
        bufs["gray8"] = _dev(np.full(n, FILL_B, np.uint8), offset)
    if "stats" in want:
        bufs["stats"] = _dev(np.full(4, FILL_F, np.float32), offset)
    torch.cuda.synchronize()
    p = capi.make_pgm_params(W, H, smooth_side, max_side, contrast, gamma, max_value)
    ctx.pgm_device(p, _ptr(src, offset), _ptr(pm, offset), _ptr(bufs.get("smoothed"), offset),
                   _ptr(bufs.get("gray8"), offset), _ptr(bufs.get("stats"), offset), stream)
    ctx.wait()
    torch.cuda.synchronize()
    assert np.array_equal(dr.bits(src.cpu().numpy()[offset:]), dr.bits(px).reshape(-1)), "input was written"
    out = {}
    for k, t in bufs.items():
        h = t.cpu().numpy()
        assert (h[:offset] == (FILL_B if k == "gray8" else FILL_F)).all(), (k, "slack was written")
        out[k] = h[offset:]
    return out


def assert_pgm(got, ref, tag=None):
    for k in got:
        (_same_b if k == "gray8" else _same_f)(got[k], ref[k], (tag, k))


# ---- 1. logf -------------------------------------------------------------------
def _assert_logf(gpu_ctx, x):
    _same_f(gpu_ctx.logf_device(x), capi.logf_host(x), "logf")


def _logf_sweep(gpu_ctx, lo, hi, stride):
    for s in range(lo, hi + 1, CHUNK * stride):
        _assert_logf(gpu_ctx, pr.floats(s, min(hi, s + CHUNK * stride - 1), stride))


def test_logf_device_equals_host(gpu_ctx):
    """The device's logf_ against the library's host build of the same source
    (equal to libm there, tests/test_pgm_cpu.py): every float of [1, 500], every
    61st pattern of (500, FLT_MAX], the edges, and the stated NaN outside."""
    _logf_sweep(gpu_ctx, pr.ONE, pr.B500, 1)
    _logf_sweep(gpu_ctx, pr.B500 + 1, pr.FLT_MAX, 61)
    _assert_logf(gpu_ctx, pr.logf_edges())
    out = np.array([0x3f7fffff, 0, 0x80000000, 1, 0xbf800000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001],
                   np.uint32).view(np.float32)
    assert (dr.bits(gpu_ctx.logf_device(out)) == 0x7fc00000).all()
    assert gpu_ctx.logf_device(np.zeros(0, np.float32)).size == 0


if EXHAUSTIVE:  # IPT_EXHAUSTIVE=1, as in tests/test_math_exhaustive.py
    @pytest.mark.slow
    def test_logf_device_equals_host_exhaustive(gpu_ctx):
        """All 1 065 353 216 floats of [1, FLT_MAX]."""
        _logf_sweep(gpu_ctx, pr.ONE, pr.FLT_MAX, 1)


# ---- 2. ipt_smooth_device ---------------------------------------------------------
def run_smooth(ctx, px, W, H, side, form):
    """form: "out" (out of place), "in" (dev_out == dev_in), "max" (dev_out
    NULL). Returns (pixels after the call, max_value)."""
    import torch

    src = _dev(np.asarray(px, np.float32))
    out = _dev(np.full(W * H, FILL_F, np.float32)) if form == "out" else None
    mx = _dev(np.full(1, FILL_F, np.float32))
    torch.cuda.synchronize()
    ctx.smooth_device(_ptr(src), _ptr(src) if form == "in" else _ptr(out), W, H, side, _ptr(mx))
    ctx.wait()
    torch.cuda.synchronize()
    after = src.cpu().numpy()
    if form != "in":
        assert np.array_equal(dr.bits(after), dr.bits(px).reshape(-1)), "input was written"
    return (out.cpu().numpy() if form == "out" else after), mx.cpu().numpy()[0]


def assert_smooth(ctx, px, W, H, side, tag=None):
    ref, rmx = pr.smooth(px, W, H, side)
    for form in ("out", "in", "max"):
        got, mx = run_smooth(ctx, px, W, H, side, form)
        _same_f(got, ref if form != "max" else px, (tag, W, H, side, form))
        assert dr.bits(mx)[0] == dr.bits(rmx)[0], (tag, W, H, side, form, mx, rmx)
    return ref, rmx


SMOOTH_SHAPES = [(1, 1, 2), (1, 7, 2), (7, 1, 2), (2, 2, 2), (4, 4, 5), (5, 5, 5), (257, 3, 2), (257, 3, 3),
                 (513, 6, 2), (513, 6, 3), (300, 9, 5), (37, 23, 0), (37, 23, 64)]


@pytest.mark.parametrize("W,H,side", SMOOTH_SHAPES, ids=[f"{W}x{H}_side{s}" for W, H, s in SMOOTH_SHAPES])
def test_smooth_device_shapes(gpu_ctx, W, H, side):
    """Sizes below, at and above the filter's side, and rows wider than one and
    two workgroups, where a pixel reads the previous block's columns; the three
    forms of the call."""
    img = pr.random_plane(W, H, 100 + W)
    ref, rmx = assert_smooth(gpu_ctx, img, W, H, side)
    qualifies = max(W - side + 1, 0) * max(H - side + 1, 0) if side >= 2 else 0
    assert int((dr.bits(ref) != dr.bits(img)).sum() > 0) == int(qualifies > 0 and W * H > 1)
    assert (rmx > 0) == (qualifies > 0)


def test_smooth_device_odd_planes(gpu_ctx):
    """All negative: the maximum stays +0. One NaN: it spreads through the sums
    of the windows that hold it and never becomes the maximum. One +inf: it does."""
    W, H = 37, 23
    base = pr.random_plane(W, H, 7)
    neg = (-base - np.float32(0.25)).astype(np.float32)
    nan, inf = base.copy(), base.copy()
    nan[5 * W + 11] = np.nan
    inf[9 * W + 20] = np.inf
    for side in (2, 5):
        ref, rmx = assert_smooth(gpu_ctx, neg, W, H, side, "negative")
        assert dr.bits(rmx)[0] == 0 and (ref[(side - 1) * W + side - 1:] < 0).all()
        ref, rmx = assert_smooth(gpu_ctx, nan, W, H, side, "nan")
        assert int(np.isnan(ref).sum()) == side * side and rmx > 0 and not np.isnan(rmx)
        ref, rmx = assert_smooth(gpu_ctx, inf, W, H, side, "inf")
        assert np.isinf(rmx) and int(np.isinf(ref).sum()) == side * side


def test_smooth_device_matches_reference_fixture(gpu_ctx):
    """tests/golden/ref_smooth.bin: the compiled reference's smooth and
    computeSmoothedMax."""
    for W, H, side, inp, sm, mx_s, mx_c in pr.smooth_golden_cases():
        got, mx = run_smooth(gpu_ctx, inp, W, H, side, "out")
        _same_f(got, sm, (W, H, side))
        assert dr.bits(mx)[0] == dr.bits(mx_s)[0]
        got, mx = run_smooth(gpu_ctx, inp, W, H, side, "in")
        _same_f(got, sm, (W, H, side, "in place"))
        _, mx = run_smooth(gpu_ctx, inp, W, H, side, "max")
        assert dr.bits(mx)[0] == dr.bits(mx_c)[0]


# ---- 3. ipt_pgm_device ---------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(37, 23), (300, 9)])
def test_pgm_device_max_rules(gpu_ctx, W, H):
    """Which max_value n_val divides by: the first matching rule of ipt_capi.h."""
    img = pr.random_plane(W, H, 200 + W)
    pmax = (pr.random_plane(W, H, 300 + W) * np.float32(3.0)).astype(np.float32)
    given = 2.5
    seen = []
    for tag, kw in (("1_window", dict(smooth_side=2, max_side=5)),
                    ("1_window_alone", dict(max_side=5)),
                    ("1_window_over_all", dict(smooth_side=2, max_side=5, pixel_max=pmax, max_value=given)),
                    ("2_smooth", dict(smooth_side=2)),
                    ("2_smooth_over_fold", dict(smooth_side=3, pixel_max=pmax, max_value=given)),
                    ("3_fold", dict(pixel_max=pmax)),
                    ("3_fold_over_given", dict(pixel_max=pmax, max_value=given)),
                    ("4_given", dict(max_value=given))):
        ref = pr.pgm_ref(img, W, H, **kw)
        assert_pgm(run_pgm(gpu_ctx, img, W, H, **kw), ref, tag)
        assert len(np.unique(ref["gray8"])) > 20, tag
        seen.append(dr.bits(ref["stats"])[0])
        if "smooth_side" not in kw:
            _same_f(ref["smoothed"], img, tag)
    assert len(set(seen)) == 6  # window, window alone, smooth 2, smooth 3, fold, given: six different maxima
    # a stage nobody asked for: every output alone
    ref = pr.pgm_ref(img, W, H, 2, 5)
    for k in ("smoothed", "gray8", "stats"):
        assert_pgm(run_pgm(gpu_ctx, img, W, H, 2, 5, want=(k,)), ref, ("alone", k))


def test_pgm_device_table(gpu_ctx):
    """The issue's table of odd inputs as 10 x 1 images (contrast 500, gamma 0.6)."""
    vals = np.array(pr.TABLE_VAL, np.float32)
    for mx in pr.TABLE_MAX:
        got = run_pgm(gpu_ctx, vals, vals.size, 1, max_value=mx)
        _same_b(got["gray8"], np.array(pr.table_want(mx), np.uint8), mx)
        assert_pgm(got, pr.pgm_ref(vals, vals.size, 1, max_value=mx), mx)
    # a zero maximum out of the fold: nothing in pixel_max is positive
    pm = np.array([-1.0, -0.0, 0.0, np.nan, -np.inf] * 2, np.float32)
    got = run_pgm(gpu_ctx, vals, vals.size, 1, pixel_max=pm)
    assert dr.bits(got["stats"])[0] == 0
    _same_b(got["gray8"], np.array(pr.table_want(0.0), np.uint8), "fold 0")
    pm[3] = np.inf
    got = run_pgm(gpu_ctx, vals, vals.size, 1, pixel_max=pm)
    assert np.isinf(got["stats"][0]) and not got["gray8"].any()


@pytest.mark.parametrize("n", [1, 3, 1023, 1025, 4 * 256 * 3 + 1])
def test_pgm_device_counts_and_unaligned_buffers(gpu_ctx, n):
    """Pixel counts around the vector width and the workgroup's span, every
    buffer one element past its allocation: the vector loads and stores must
    fall back and touch nothing outside."""
    img = pr.random_plane(n, 1, 400 + n)
    pmax = (img * np.float32(1.5)).astype(np.float32)
    for offset in (0, 1):
        assert_pgm(run_pgm(gpu_ctx, img, n, 1, pixel_max=pmax, offset=offset), pr.pgm_ref(img, n, 1, pixel_max=pmax),
                   (n, offset))
    if n >= 1023:  # as rows of 3, 5 or 7: smooth and the window maximum at these counts
        W = next(w for w in (3, 5, 7) if n % w == 0)
        H = n // W
        assert_pgm(run_pgm(gpu_ctx, img, W, H, 2, 3, offset=1), pr.pgm_ref(img, W, H, 2, 3), (W, H, "smooth"))


def _domain_plane(stride):
    v = pr.floats(pr.ONE, pr.B500, stride)
    return v, pr.n_val(v, 500.0)


def test_pgm_device_logf_domain(gpu_ctx):
    """The plane holding every 61st float of [1, 500] with max_value 500: adj
    walks n_val's whole logf domain, fn powf's [0, 1]."""
    v, ref = _domain_plane(61)
    assert v.size > 1_200_000 and ref[0] == 0 and ref[-1] == 255 and len(np.unique(ref)) == 256
    got = run_pgm(gpu_ctx, v, v.size, 1, max_value=500.0, want=("gray8",))
    _same_b(got["gray8"], ref, "domain")


if EXHAUSTIVE:
    @pytest.mark.slow
    def test_pgm_device_logf_domain_exhaustive(gpu_ctx):
        """Every float of [1, 500] as one 75.1 M-pixel plane."""
        v, ref = _domain_plane(1)
        got = run_pgm(gpu_ctx, v, v.size, 1, max_value=500.0, want=("gray8",))
        _same_b(got["gray8"], ref, "domain")


@pytest.mark.parametrize("contrast,gamma", pr.PAIRS)
def test_pgm_device_contrast_gamma(gpu_ctx, contrast, gamma):
    W, H = 37, 23
    img = pr.random_plane(W, H, 11)
    ref = pr.pgm_ref(img, W, H, 2, 5, contrast, gamma)
    assert_pgm(run_pgm(gpu_ctx, img, W, H, 2, 5, contrast, gamma), ref, (contrast, gamma))
    assert ref["gray8"].max() == 255 and len(np.unique(ref["gray8"])) >= 2


def test_host_pgm_equals_device_and_python_defaults(gpu_ctx):
    W, H = 53, 21
    img = pr.random_plane(W, H, 13)
    pmax = (img * np.float32(2.0)).astype(np.float32)
    for kw in (dict(smooth_side=2, max_side=5), dict(pixel_max=pmax), dict(max_value=1.25),
               dict(smooth_side=2, max_side=5, contrast=2.0, gamma=0.5)):
        assert_pgm(gpu_ctx.pgm(img, W, H, **kw), run_pgm(gpu_ctx, img, W, H, **kw), kw.keys())


# ---- 4. stream order -------------------------------------------------------------------
def test_stream_order_after_async_render(gpu_ctx, oracle):
    """render_device_async then pgm_device (smooth 2, smoothed max 5) on one
    torch stream with no host wait between them: the PGM reads the finished
    plane, and equals pgm_ref of the oracle's."""
    import oracle_binding
    import torch

    W, H = 64, 64
    desc = scenes.make_scene_box()
    gpu_ctx.upload_scene(desc)
    p = capi.make_params(W, H, 2, n_rays=4, depth_max=3)
    A = torch.zeros(4, H, W, dtype=torch.float32, device="cuda")
    g8 = torch.full((W * H,), FILL_B, dtype=torch.uint8, device="cuda")
    sm = torch.full((W * H,), FILL_F, dtype=torch.float32, device="cuda")
    st = torch.full((4,), FILL_F, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        gpu_ctx.render_device_async(p, *(A[i].data_ptr() for i in range(4)), s.cuda_stream)
        gpu_ctx.pgm_device(capi.make_pgm_params(W, H, 2, 5), A[0].data_ptr(), A[3].data_ptr(), sm.data_ptr(),
                           g8.data_ptr(), st.data_ptr(), s.cuda_stream)
    s.synchronize()
    got = {"smoothed": sm.cpu().numpy(), "gray8": g8.cpu().numpy(), "stats": st.cpu().numpy()}
    gpu_ctx.wait()
    ov, oc = oracle_binding.render_values(desc, p)
    plane = oracle_binding.accumulate(ov, oc)
    assert plane["pixels"].max() > 0
    _same_f(A[0].cpu().numpy().reshape(-1), plane["pixels"], "plane")
    assert_pgm(got, pr.pgm_ref(plane["pixels"], W, H, 2, 5), "after render")
    assert len(np.unique(got["gray8"])) > 50


def _queue(ctx, src, g8, W, H, stream):
    """ipt_pgm_device on `stream` with NULL smoothed (the context's scratch
    carries the smoothed plane); queues only, no synchronisation of any kind."""
    ctx.pgm_device(capi.make_pgm_params(W, H, 64, 64), src.data_ptr(), None, None, g8.data_ptr(), None,
                   stream.cuda_stream)


def test_two_streams_share_the_scratch():
    """Two calls on two streams with no host wait between them: the second must
    run behind the first (hipStreamWaitEvent on the context's event), because
    both use the context's scalars and smoothed plane. L (320 x 320) and S
    (96 x 80) with sides 64, the longest kernels the call allows, alternate
    over four pairs after a warm-up that grows the scratch, so that no call
    takes the allocating path, which waits on the host; the warm-up's second
    call at the same size runs through the scratch as it stands.

    An ordering test is probabilistic: it cannot prove that the wait is there,
    it only fails with good likelihood when it is missing."""
    import torch

    cases = {"L": (320, 320, pr.random_plane(320, 320, 21)), "S": (96, 80, pr.random_plane(96, 80, 22))}
    refs = {k: pr.pgm_ref(img, W, H, 64, 64)["gray8"] for k, (W, H, img) in cases.items()}
    assert all(len(np.unique(r)) > 20 for r in refs.values())
    ctx = capi.Context(0)
    try:
        src = {k: torch.from_numpy(img).cuda() for k, (W, H, img) in cases.items()}
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        WL, HL, _ = cases["L"]
        warm = [torch.full((WL * HL,), FILL_B, dtype=torch.uint8, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        for w in warm:  # the first call grows the scratch; the second allocates nothing
            _queue(ctx, src["L"], w, WL, HL, s1)
            ctx.wait()
        out = []
        for first, second in (("L", "S"), ("S", "L"), ("L", "S"), ("S", "L")):
            pair = [(key, torch.full((cases[key][0] * cases[key][1],), FILL_B, dtype=torch.uint8, device="cuda"))
                    for key in (first, second)]
            torch.cuda.synchronize()
            for (key, g8), stream in zip(pair, (s1, s2)):
                _queue(ctx, src[key], g8, cases[key][0], cases[key][1], stream)
            ctx.wait()
            torch.cuda.synchronize()
            out += pair
        for w in warm:
            _same_b(w.cpu().numpy(), refs["L"], "warm")
        for i, (key, g8) in enumerate(out):
            _same_b(g8.cpu().numpy(), refs[key], (i, key))
    finally:
        ctx.close()


def test_scratch_regrowth():
    """small, large, small through the context's scratch (NULL smoothed), and an
    in-place smooth that shares it."""
    ctx = capi.Context(0)
    try:
        small, big = pr.random_plane(64, 48, 31), pr.random_plane(300, 200, 32)
        first = run_pgm(ctx, small, 64, 48, 2, 5, want=("gray8",))
        second = run_pgm(ctx, big, 300, 200, 2, 5, want=("gray8",))
        got, mx = run_smooth(ctx, big, 300, 200, 3, "in")
        third = run_pgm(ctx, small, 64, 48, 2, 5, want=("gray8",))
        assert_pgm(first, pr.pgm_ref(small, 64, 48, 2, 5))
        assert_pgm(second, pr.pgm_ref(big, 300, 200, 2, 5))
        _same_f(got, pr.smooth(big, 300, 200, 3)[0], "in place")
        assert_pgm(third, first)
    finally:
        ctx.close()


# ---- 5. argument errors -----------------------------------------------------------------
def test_argument_errors(gpu_ctx):
    """Every rule of ipt_capi.h returns its code, and no buffer is touched."""
    import torch

    lib, h = gpu_ctx.lib, gpu_ctx.h
    W, H = 8, 6
    tpx = torch.zeros(W * H + 8, dtype=torch.float32, device="cuda")
    tother = torch.zeros(W * H + 8, dtype=torch.float32, device="cuda")
    tg8 = torch.zeros(W * H, dtype=torch.uint8, device="cuda")
    tone = torch.zeros(4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    px, other, g8, one = (t.data_ptr() for t in (tpx, tother, tg8, tone))
    INV, UNS = capi.IPT_E_INVALID, capi.IPT_E_UNSUPPORTED

    def smooth(src=px, out=other, w=W, hh=H, side=2, mx=one):
        return lib.ipt_smooth_device(h, src, out, w, hh, side, mx, None)

    assert smooth(src=None) == INV
    assert smooth(w=0) == INV and smooth(hh=-1) == INV and smooth(side=-1) == INV
    assert smooth(out=px + 4) == INV                             # a shifted overlap
    assert smooth(mx=px + 8) == INV and smooth(mx=other) == INV
    assert smooth(side=1) == UNS and smooth(side=65) == UNS
    assert smooth(w=65536, hh=32769, out=None, mx=None) == UNS   # more than 2^31 pixels

    def pgm(src=px, pm=None, sm=None, out=g8, st=None, **kw):
        q = capi.make_pgm_params(**{"width": W, "height": H, **kw})
        return lib.ipt_pgm_device(h, C.byref(q), src, pm, sm, out, st, None)

    assert lib.ipt_pgm_device(h, None, px, None, None, g8, None, None) == INV
    assert pgm(src=None) == INV
    assert pgm(width=0) == INV and pgm(height=-3) == INV
    assert pgm(smooth_side=-1) == INV and pgm(max_side=-2) == INV
    assert pgm(sm=px) == INV and pgm(sm=px + 4 * (W * H - 1)) == INV
    assert pgm(st=px + 16) == INV and pgm(pm=other, sm=other) == INV
    assert pgm(sm=other, st=other + 4) == INV
    assert pgm(smooth_side=1) == UNS and pgm(max_side=1) == UNS
    assert pgm(smooth_side=65) == UNS and pgm(max_side=65) == UNS
    assert pgm(flags=1) == UNS
    assert pgm(width=65536, height=32769, out=None) == UNS
    for c in (1.0, 0.5, -3.0, np.inf, np.nan):
        assert pgm(contrast=c) == UNS, c
    for g in (0.0, -0.6, 1.0, 2.0, np.inf, np.nan):
        assert pgm(gamma=g) == UNS, g
    # the host form validates the same way
    hpx, hg8 = np.zeros(W * H, np.float32), np.zeros(W * H, np.uint8)
    q = capi.make_pgm_params(W, H, smooth_side=1)
    assert lib.ipt_pgm(h, C.byref(q), hpx.ctypes.data, None, None, hg8.ctypes.data, None) == UNS
    q = capi.make_pgm_params(W, H)
    assert lib.ipt_pgm(h, C.byref(q), None, None, None, hg8.ctypes.data, None) == INV
    with pytest.raises(capi.IptError) as e:
        gpu_ctx.pgm(hpx, W, H, contrast=1.0)
    assert e.value.code == UNS
    gpu_ctx.wait()
    torch.cuda.synchronize()
    for t in (tpx, tother, tg8, tone):
        assert not t.cpu().numpy().any()


# ---- 6. CLI -------------------------------------------------------------------------------
def test_cli_gpu_display_pgm_is_identical(tmp_path):
    """ipt_render --pgm with main.cpp's sequence (smooth 2, smoothed max 5):
    the file written from GpuRenderer::pgm's bytes equals the host n_val loop's."""
    exe = ge.build_host()
    args = [str(exe), "--scene", "box", "--spp", "2", "--width", "40", "--height", "24", "--out", "",
            "--smooth", "2", "--smoothed-max", "5"]
    subprocess.run(args + ["--pgm", str(tmp_path / "cpu.pgm")], check=True, capture_output=True, timeout=120)
    subprocess.run(args + ["--gpu-display", "--pgm", str(tmp_path / "gpu.pgm")], check=True, capture_output=True,
                   timeout=120)
    a, b = (tmp_path / "cpu.pgm").read_bytes(), (tmp_path / "gpu.pgm").read_bytes()
    assert a == b
    head = a.split(b"\n", 3)
    assert head[:3] == [b"P2", b"40 24", b"255"]
    v = np.array(head[3].split(), np.int64)
    assert v.size == 40 * 24 and v.max() == 255 and len(np.unique(v)) > 20
    # without the smoothed maximum the plane's own max_value divides: other bytes
    subprocess.run(args[:-2] + ["--gpu-display", "--pgm", str(tmp_path / "plain.pgm")], check=True,
                   capture_output=True, timeout=120)
    subprocess.run(args[:-2] + ["--pgm", str(tmp_path / "plain_cpu.pgm")], check=True, capture_output=True,
                   timeout=120)
    assert (tmp_path / "plain.pgm").read_bytes() == (tmp_path / "plain_cpu.pgm").read_bytes() != a
