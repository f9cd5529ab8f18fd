"""What the GPU tests of temporal reprojection share: device copies of a
case, ipt_reproject_device on them, and the comparison with
tests/reproject_cases.py's restatement, bit for bit on the three planes and
the stats (tests/test_gpu_reproject.py, tests/test_gpu_reproject_edges.py)."""
import numpy as np
import torch

import adaptive_cases as ac
import denoise_cases as dn
import reproject_cases as rc
from ipt_amd import capi

F = np.float32
DEV = torch.device("cuda", 0)
CANARY = 777.0
STATS_JUNK = 0x25a5a5a5  # the call zeroes the stats itself


def _t(a):
    a = np.array(a, order="C")  # (a writable copy: the cases' arrays are read-only)
    if a.dtype == capi.GuideRecord:
        a = a.reshape(-1).view(np.uint8)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)


def _h(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def _outs(n):
    return (torch.full((n,), CANARY, dtype=torch.float32, device=DEV),
            torch.full((n,), 0x5a5a5a5a, dtype=torch.int32, device=DEV),
            torch.full((n,), CANARY, dtype=torch.float32, device=DEV),
            torch.full((4,), STATS_JUNK, dtype=torch.int32, device=DEV))


def _reproject(ctx, case, W, H, plane=rc.GRID, stats=True, **kw):
    """ipt_reproject_device on device copies of the case; (pixels, counters,
    m2, stats or None) on the host."""
    px, cn, m2, pg, cg, cam = case
    rp = capi.make_reproject_params(W, H, cam, flags=ac.FLAG[plane], **kw)
    ins = [_t(np.asarray(px, F)), _t(np.asarray(cn, np.uint32)), _t(np.asarray(m2, F)), _t(pg), _t(cg)]
    opx, ocn, om2, st = _outs(W * H)
    torch.cuda.synchronize()
    ctx.reproject_device(rp, *(t.data_ptr() for t in ins), opx.data_ptr(), ocn.data_ptr(), om2.data_ptr(),
                         st.data_ptr() if stats else None)
    ctx.wait()
    torch.cuda.synchronize()
    return _h(opx), _h(ocn), _h(om2), (_h(st) if stats else None)


def _equal(got, ref, what=""):
    for k, name in ((0, "pixels"), (2, "m2")):
        bad = ~dn.same(got[k], ref[k])
        assert not bad.any(), (what, name, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())
    bad = got[1] != ref[1]
    assert not bad.any(), (what, "counters", int(bad.sum()), np.flatnonzero(bad)[:8].tolist())
    if got[3] is not None:
        assert got[3].tolist() == ref[3].tolist(), (what, "stats")


def _check(ctx, case, W, H, plane=rc.GRID, what="", **kw):
    ref = rc.reproject(*case[:5], W, H, case[5], plane, **kw)
    _equal(_reproject(ctx, case, W, H, plane, **kw), ref, what)
    return ref
