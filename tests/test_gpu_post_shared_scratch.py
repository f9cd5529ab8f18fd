"""The post-processing entry points through one context's scratch, back to
back: display, PGM, display statistics, denoise, adapt, smooth and display
again, alternating between two streams with no synchronisation before the end.
Every per-entry test shares the scratch with itself; here the different entry
points meet on it (ipt_post.hip's post_begin / post_queued), across a regrowth
(67 x 35, then 300 x 75) and small after large. Every output has its own buffer
and is compared bit for bit with the CPU restatements of the per-entry tests.

300 x 75 crosses a denoiser lattice tile and is more than one kCompactSpan
block; 67 x 35 is smaller than a block row."""
import numpy as np
import pytest

import adaptive_cases as ac
import denoise_cases as dn
import display_cases as dc
import display_ref as dr
import pgm_ref as pr
import stats_ref as sr
from ipt_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32
SMALL, LARGE = (67, 35), (300, 75)
CUTOFF = dc.STREAM_CUTOFF
ADAPT = dict(min_count=4, rel_tol=0.25, abs_tol=1e-3)


def bright_plane(W, H, seed, hot):
    """display_cases' dim plane with `hot` pixels above the cutoff."""
    rng = np.random.default_rng(seed)
    img = dc.dim(rng, W * H)
    img[rng.choice(W * H, hot, replace=False)] = (rng.random(hot, dtype=F) * 40 + F(51.5)).astype(F)
    return img


def test_every_entry_point_on_one_scratch(oracle):
    import torch

    dev = torch.device("cuda", 0)

    def up(a):
        a = np.array(a, order="C")
        if a.dtype == capi.GuideRecord:
            a = a.reshape(-1).view(np.uint8)
        return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)

    def new(n, dtype, fill):
        return torch.full((n,), fill, dtype=dtype, device=dev)

    def host(t):
        a = t.cpu().numpy()
        return a.view(np.uint32) if a.dtype == np.int32 else a

    (WS, HS), (WL, HL) = SMALL, LARGE
    nS, nL = WS * HS, WL * HL
    small_a, small_b = bright_plane(WS, HS, 101, 30), bright_plane(WS, HS, 102, 45)
    large = bright_plane(WL, HL, 103, 200)
    px, cn, m2 = dn.random_plane(WL, HL, 11)
    guides = dn.crease_guides(WL, HL)
    rank = sr.white_rank_for(WL, HL, 0.95)
    assert int((small_a > CUTOFF).sum()) == 30 and int((large > CUTOFF).sum()) == 200

    d_small_a, d_small_b, d_large = up(small_a), up(small_b), up(large)
    d_px, d_cn, d_m2, d_g = up(px), up(cn), up(m2), up(guides)
    d_inplace = up(large)
    g8_1, g8_7 = new(nS, torch.uint8, 9), new(nS, torch.uint8, 9)
    pgm_g8, pgm_stats = new(nS, torch.uint8, 9), new(4, torch.float32, -7.0)
    st_g8, st_hist, st_stats = new(nL, torch.uint8, 9), new(16, torch.int32, -1), new(4, torch.float32, -7.0)
    dn_out, dn_var = new(nL, torch.float32, 777.0), new(nL, torch.float32, 777.0)
    ad_mask, ad_stats = new(nL, torch.uint8, 9), new(4, torch.int32, -1)
    sm_max = new(1, torch.float32, -7.0)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()

    ctx = capi.Context(0)
    try:
        h1, h2 = s1.cuda_stream, s2.cuda_stream
        # queues only: no synchronisation of any kind before the end
        ctx.display_device(capi.make_display_params(WS, HS, CUTOFF), d_small_a.data_ptr(), g8_1.data_ptr(),
                           stream=h1)
        ctx.pgm_device(capi.make_pgm_params(WS, HS, smooth_side=2, max_side=5), d_small_a.data_ptr(), None, None,
                       pgm_g8.data_ptr(), pgm_stats.data_ptr(), h2)
        ctx.display_stats_device(capi.make_display_stats_params(WL, HL, CUTOFF, 16, rank), d_large.data_ptr(), None,
                                 None, st_g8.data_ptr(), st_hist.data_ptr(), st_stats.data_ptr(), h1)
        ctx.denoise_device(capi.make_denoise_params(WL, HL, iterations=3), d_px.data_ptr(), d_cn.data_ptr(),
                           d_m2.data_ptr(), d_g.data_ptr(), dn_out.data_ptr(), dn_var.data_ptr(), h2)
        ctx.adapt_device(capi.make_adapt_params(WL, HL, **ADAPT), d_px.data_ptr(), d_cn.data_ptr(), d_m2.data_ptr(),
                         ad_mask.data_ptr(), ad_stats.data_ptr(), h1)
        ctx.smooth_device(d_inplace.data_ptr(), d_inplace.data_ptr(), WL, HL, 3, sm_max.data_ptr(), h2)
        ctx.display_device(capi.make_display_params(WS, HS, CUTOFF), d_small_b.data_ptr(), g8_7.data_ptr(),
                           stream=h2)
        s1.synchronize()
        s2.synchronize()

        def same(got, ref, what):
            got, ref = np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1)
            if got.dtype == F:
                got, ref = dr.bits(got), dr.bits(ref)
            bad = got != ref
            assert got.shape == ref.shape and not bad.any(), (what, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())

        same(host(g8_1), dr.display_ref(small_a, WS, HS, CUTOFF)["gray8"], "1 display")
        ref = pr.pgm_ref(small_a, WS, HS, smooth_side=2, max_side=5)
        same(host(pgm_g8), ref["gray8"], "2 pgm gray8")
        same(host(pgm_stats), ref["stats"], "2 pgm stats")
        ref = sr.stats_ref(large, WL, HL, CUTOFF, 16, rank)
        same(host(st_g8), ref["gray8"], "3 stats gray8")
        same(host(st_hist), ref["hist"], "3 stats hist")
        same(host(st_stats), ref["stats"], "3 stats stats")
        ro, rv = dn.denoise(px, cn, m2, guides, WL, HL, iterations=3)
        assert dn.same(host(dn_out), ro).all() and dn.same(host(dn_var), rv).all(), "4 denoise"
        mask, stats = ac.adapt(px, cn, m2, WL, HL, **ADAPT)
        assert 0 < stats[0] < nL and stats[1] > 0  # some pixels active, some of them starved, some settled
        same(host(ad_mask), mask, "5 adapt mask")
        same(host(ad_stats), stats, "5 adapt stats")
        sm, mx = pr.smooth(large, WL, HL, 3)
        same(host(d_inplace), sm, "6 smooth")
        same(host(sm_max), np.array([mx], F), "6 smooth max")
        same(host(g8_7), dr.display_ref(small_b, WS, HS, CUTOFF)["gray8"], "7 display")
        # the inputs were read only
        same(host(d_small_a), small_a, "input")
        same(host(d_large), large, "input")
        same(host(d_px), px, "input")
    finally:
        ctx.close()
