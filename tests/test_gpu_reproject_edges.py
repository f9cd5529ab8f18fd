"""Temporal reprojection on the device where its definition's comparisons land
on equality, against tests/reproject_cases.py's restatement bit for bit on the
three planes and the stats: the dyadic lattice under every shift (whole, half
and quarter pixels, fx == -1 and fx == W, a plane distance of exactly sigma_z,
n.n_q of exactly normal_min, counters at the cap, denormal and near-FLT_MAX
m2), the same lattice one and two ulp off, cameras at the ends of step 2,
frames of one and two pixels, out_m2 = +inf where the definition overflows,
planes at addresses that are no multiple of 8, and the host form.
tests/test_reproject_edges_cpu.py pins, without a GPU, that these cases reach
every such event and that the restatement is the header's definition there."""
import numpy as np
import pytest
import torch

import adaptive_cases as ac
import denoise_cases as dn
import drift_cases as dc
import reproject_cases as rc
from ipt_amd import capi
from reproject_gpu import CANARY, DEV, _check, _equal, _reproject, _t

pytestmark = pytest.mark.gpu

F = np.float32
SHIFTS = tuple(name for name, _ in rc.LATTICE_SHIFTS)
TINY_SHIFTS = ((0.0, 0.0), (0.5, 0.5), (-0.5, -0.5), (0.0, -1.0))


def _params(mc=rc.LATTICE["max_count"]):
    return dict(rc.LATTICE, max_count=mc)


@pytest.mark.parametrize("plane", ac.PLANES)
@pytest.mark.parametrize("max_count", rc.LATTICE_MAX_COUNTS)
@pytest.mark.parametrize("frame", rc.LATTICE_FRAMES, ids=lambda f: "%dx%d" % f)
def test_lattice_shifts(gpu_ctx, frame, max_count, plane):
    """Every shift of LATTICE_SHIFTS; 32 x 16 already spans two workgroups."""
    W, H = frame
    reused = 0
    for shift in SHIFTS:
        case = rc.lattice_case(W, H, shift, plane, max_count=max_count)
        reused += int(_check(gpu_ctx, case, W, H, plane, (shift, plane), **_params(max_count))[3][0])
    assert reused > W * H


@pytest.mark.parametrize("plane", ac.PLANES)
@pytest.mark.parametrize("frame", rc.NEAR_FRAMES, ids=lambda f: "%dx%d" % f)
def test_near_lattice(gpu_ctx, frame, plane):
    """fx and fy one and two ulp either side of -1, the integers and W; 37 x 23
    and 131 x 67 are no powers of two, so (a / t + 0.5) W rounds."""
    W, H = frame
    for shift in SHIFTS:
        _check(gpu_ctx, rc.near_lattice_case(W, H, shift, plane), W, H, plane, (shift, plane), **_params())


@pytest.mark.parametrize("plane", ac.PLANES)
def test_camera_edges(gpu_ctx, plane):
    """A zero, a denormal, a 2^60 and a 2^-60 direction, a position of 3e38 and
    one of +inf, a NaN right, zero up and right, a camera in the guides' plane:
    step 2 says where each ends, and the kernel ends there too."""
    W, H = 32, 16
    planes = rc.lattice_case(W, H, "quarter_xy", plane)[:5]
    surface = int(((planes[4]["kind"] & 3) == 1).sum())
    seen = {}
    for name, cam in rc.camera_edge_cases(W, H).items():
        ref = _check(gpu_ctx, planes + (cam,), W, H, plane, (name, plane), **_params())
        seen[name] = ref[3].tolist()
    # direction 0: c = 0 and dd = 0, t = 0 / 0 is NaN and !(t > 0): every surface pixel is "disoccluded"
    assert seen["zero_direction"] == [0, surface, W * H - surface, 0]
    assert seen["in_plane"] == seen["nan_right"] == seen["inf_position"] == seen["zero_direction"]
    # t = +inf or a = b = 0: a / t = 0 and every pixel lands on the frame's centre, so all of them
    # share their four taps and their class; on planes whose every tap passes, all are reused
    benign = rc.lattice_case(W, H, "none", plane, benign=True)[:5]
    for name in ("denormal_direction", "position_3e38", "zero_up_right"):
        assert seen[name][0] in (0, surface) and seen[name][0] + seen[name][1] == surface
        ref = _check(gpu_ctx, benign + (rc.camera_edge_cases(W, H)[name],), W, H, plane, (name, "benign"), **_params())
        assert ref[3].tolist() == [surface, 0, W * H - surface, 0]
    # the scaled directions project as the lattice's own camera
    own = rc.reproject(*planes, W, H, rc.lattice_camera(W, H), plane, **_params())[3].tolist()
    assert seen["direction_2p60"] == seen["direction_2m60"] == own and own[0] > W * H // 4


@pytest.mark.parametrize("plane", ac.PLANES)
def test_tiny_lattice_frames(gpu_ctx, plane):
    """1 x 1, 2 x 1, 1 x 2, 2 x 2, 4 x 2 and 1 x 8: most taps leave the frame,
    and under the Grid map a frame of two rows has one source row."""
    for W, H in rc.TINY_LATTICE_FRAMES:
        for shift in TINY_SHIFTS:
            ref = _check(gpu_ctx, rc.constant_lattice_case(W, H, shift, plane), W, H, plane, (W, H, shift),
                         **_params())
            if shift[1] != -1.0:  # (constant planes: every pixel with a nominal source is reused)
                assert ref[3][0] == W * (H - 1 if plane == rc.GRID and H > 1 else H)


@pytest.mark.parametrize("plane", ac.PLANES)
def test_overflow_gives_the_definitions_infinity(gpu_ctx, plane):
    """Finite inputs that pass step 3, m2 = 3e38 at small counters: var (nf'
    (nf' - 1)) overflows and out_m2 is +inf on the device exactly where the
    definition's is (include/ipt_capi.h, step 4)."""
    W, H = 32, 16
    case = rc.lattice_case(W, H, "half_xy", plane)
    ref = rc.reproject(*case[:5], W, H, case[5], plane, **_params())
    got = _reproject(gpu_ctx, case, W, H, plane, **_params())
    inf = ref[2] == np.inf
    assert inf.sum() > 0 and (ref[4][inf] == rc.REUSED).all() and np.isfinite(ref[2][~inf]).all()
    assert np.array_equal(got[2] == np.inf, inf) and np.isfinite(got[2][~inf]).all()
    assert np.isfinite(got[0]).all()
    _equal(got, ref, plane)


def _misaligned(ctx, case, W, H, plane, **kw):
    """The call with all eight planes and the stats at odd dword offsets of one
    16-byte aligned allocation, three dwords of canary between them; the
    outputs, and the buffer before and after the call as bits."""
    n = W * H
    sizes = (n, n, n, 8 * n, 8 * n, n, n, n, 4)
    at, cursor = [], 1
    for s in sizes:
        at.append(cursor)
        cursor += s + 3
        cursor += 1 - cursor % 2
    buf = torch.full((cursor + 3,), CANARY, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0 and all(a % 2 == 1 for a in at)
    ins = (_t(np.asarray(case[0], F)), _t(np.asarray(case[1], np.uint32)), _t(np.asarray(case[2], F)), _t(case[3]),
           _t(case[4]))
    for a, s, t in zip(at, sizes, ins):
        buf[a:a + s] = t.view(torch.float32)
    before = buf.cpu().numpy().view(np.uint32).copy()
    torch.cuda.synchronize()
    rp = capi.make_reproject_params(W, H, case[5], flags=ac.FLAG[plane], **kw)
    ctx.reproject_device(rp, *(buf.data_ptr() + 4 * a for a in at))
    ctx.wait()
    torch.cuda.synchronize()
    after = buf.cpu().numpy().view(np.uint32)
    outs = [after[a:a + s] for a, s in zip(at[5:], sizes[5:])]
    written = np.zeros(after.size, bool)
    for a, s in zip(at[5:], sizes[5:]):
        written[a:a + s] = True
    return (outs[0].view(F), outs[1], outs[2].view(F), outs[3]), before, after, written


@pytest.mark.parametrize("plane", ac.PLANES)
def test_misaligned_planes(gpu_ctx, plane):
    """The header allows the planes "any alignment a float has": every buffer
    at an address that is 4 and not 0 modulo 8. The results are the aligned
    call's bits, and no byte outside the outputs changes."""
    for case, W, H, kw in ((rc.lattice_case(32, 16, "half_xy", plane), 32, 16, _params()),
                           (rc.poisoned(rc.synthetic_case("crease", 67, 35), 67, 35), 67, 35, {})):
        got, before, after, written = _misaligned(gpu_ctx, case, W, H, plane, **kw)
        _equal(got, rc.reproject(*case[:5], W, H, case[5], plane, **kw), (W, H, plane))
        assert np.array_equal(before[~written], after[~written]), (W, H, plane)
        assert (before[written] != after[written]).any()


@pytest.mark.parametrize("plane", ac.PLANES)
def test_host_form_on_edge_cases(gpu_ctx, plane):
    """ipt_reproject on a lattice case and on a camera edge case: the device
    form's bits."""
    W, H = 32, 16
    lattice = rc.lattice_case(W, H, "half_xy", plane)
    for case in (lattice, lattice[:5] + (rc.camera_edge_cases(W, H)["denormal_direction"],),
                 lattice[:5] + (rc.camera_edge_cases(W, H)["zero_direction"],)):
        rp = capi.make_reproject_params(W, H, case[5], flags=ac.FLAG[plane], **_params())
        px, cn, m2, st = gpu_ctx.reproject(rp, *case[:5])
        host = (px, cn, m2, np.array([st["reused"], st["disoccluded"], st["not_surface"], 0], np.uint32))
        dev = _reproject(gpu_ctx, case, W, H, plane, **_params())
        _equal(host, dev, plane)
        assert dn.same(host[2], dev[2]).all() and np.array_equal(dc.bits(host[0]), dc.bits(dev[0]))
        _equal(host, rc.reproject(*case[:5], W, H, case[5], plane, **_params()), plane)
