"""Inputs for the display pipeline's large-shape and edge tests, each with the
CPU-side conditions that make it discriminating. The generators are shared by
tests/test_display_cpu.py (conditions alone, no GPU) and
tests/test_gpu_display.py / tests/test_post.py (the same conditions, then the
kernels); references are computed once per process and must not be written to.

The constants restate ipt_post.hip: a compaction block owns 1024 pixels
(kCompactSpan) and bright_scan_kernel is one workgroup of 256 threads, each
owning `per = ceil(nblk / 256)` consecutive blocks."""
import functools

import numpy as np

import display_ref as dr

SPAN = 1024       # kCompactSpan
SCAN_THREADS = 256  # kPostBlock
TINY = np.float32(2.0 ** -126)  # the smallest normal float
FLT_MAX = np.float32(3.4028234663852886e38)


def dim(rng, n):
    return (rng.random(n, dtype=np.float32) * np.float32(0.49)).astype(np.float32)


# ---- A. compaction above 256 blocks ----------------------------------------
SCAN_SHAPES = [(512, 512), (257, 1024), (4096, 65), (640, 640)]  # (W, H)
SCAN_CUTOFF = 50.0
SCAN_BRIGHT = 300


def scan_geometry(n):
    """(nblk, per, threads that own a block) of bright_scan_kernel for n pixels."""
    nblk = -(-n // SPAN)
    per = -(-nblk // SCAN_THREADS)
    return nblk, per, -(-nblk // per)


def scan_positions(n):
    """The deliberate bright positions: first and last pixel of the blocks on
    either side of the scan-thread boundaries at the start, middle and end."""
    nblk, per, used = scan_geometry(n)
    blocks = {0, 1, 2, 3, nblk - 3, nblk - 2, nblk - 1}
    for k in (used // 2, used // 2 + 1):
        blocks |= {per * k - 1, per * k, per * k + 1}
    assert all(0 <= b < nblk for b in blocks)
    pos = {0, n - 1}
    for b in blocks:
        pos |= {b * SPAN, min(b * SPAN + SPAN - 1, n - 1)}
    return sorted(pos)


@functools.lru_cache(maxsize=None)
def scan_case(W, H):
    """(img, positions of the bright pixels) for one shape of SCAN_SHAPES."""
    n = W * H
    rng = np.random.default_rng(1000 + W)
    img = dim(rng, n)
    placed = scan_positions(n)
    free = np.setdiff1d(np.arange(n), placed)
    pos = np.sort(np.concatenate([placed, rng.choice(free, SCAN_BRIGHT - len(placed), replace=False)]))
    # distinct values in (51.5, 91.5), in random order along the raster
    frac = (rng.permutation(SCAN_BRIGHT) + 0.5) / SCAN_BRIGHT
    vals = (np.float32(51.5) + np.float32(40.0) * frac).astype(np.float32)
    img[pos] = vals
    img.setflags(write=False)
    return img, pos


@functools.lru_cache(maxsize=None)
def scan_ref(W, H):
    """display_ref of scan_case(W, H) after its conditions hold (needs the oracle)."""
    img, pos = scan_case(W, H)
    n = W * H
    assert len(pos) == SCAN_BRIGHT == len(set(pos.tolist())) and SCAN_BRIGHT * n <= 1.3e8
    hot = img[pos]
    assert len(np.unique(hot)) == SCAN_BRIGHT and hot.min() > 51.5 and hot.max() < 91.5
    assert int((img > SCAN_CUTOFF).sum()) == SCAN_BRIGHT and img[0] > SCAN_CUTOFF and img[n - 1] > SCAN_CUTOFF
    assert set(scan_positions(n)) <= set(pos.tolist())
    ref = dr.display_ref(img, W, H, SCAN_CUTOFF)
    # a saturated image hides the order of the halo sums
    assert (ref["processed"] < SCAN_CUTOFF).sum() > 0.5 * n
    for v in ref.values():
        v.setflags(write=False)
    return ref


# ---- B. far halos -----------------------------------------------------------
FAR_W, FAR_H, FAR_CUTOFF, FAR_VALUE = 4096, 512, 1.0, 100.0
FAR_CORNERS = [(0, 0), (FAR_W - 1, FAR_H - 1)]


def far_image(cx, cy):
    img = np.zeros(FAR_W * FAR_H, np.float32)
    img[cy * FAR_W + cx] = FAR_VALUE
    return img


def far_models(cx, cy):
    """(s, near-formula model, far-formula model) of glare(far_image): numpy
    float32 restatements of C/(0.25+r)/(0.25+r) added to the image and cut,
    with r = sqrtf((float)s) and r = (float)sqrt((double)s), s = dx^2 + dy^2."""
    img = far_image(cx, cy)
    x = np.arange(FAR_W, dtype=np.int64)[None, :] - cx
    y = np.arange(FAR_H, dtype=np.int64)[:, None] - cy
    s = (x * x + y * y).reshape(-1)
    cutoff = np.float32(FAR_CUTOFF)
    c = cutoff * np.float32(0.1 * float(np.float32(FAR_VALUE)) / float(cutoff))
    out = []
    for r in (np.sqrt(s.astype(np.float32)), np.sqrt(s.astype(np.float64)).astype(np.float32)):
        d = (np.float32(0.25) + r).astype(np.float32)
        v = (img + ((c / d).astype(np.float32) / d).astype(np.float32)).astype(np.float32)
        out.append(np.where(v < 0, np.float32(0), np.where(v > cutoff, cutoff, v)).astype(np.float32))
    return s, out[0], out[1]


@functools.lru_cache(maxsize=None)
def far_ref(cx, cy):
    ref = dr.display_ref(far_image(cx, cy), FAR_W, FAR_H, FAR_CUTOFF)
    for v in ref.values():
        v.setflags(write=False)
    return ref


# ---- C. denormals and extreme range in tone / 8-bit ------------------------
def _from_bits(b):
    return np.asarray(b, np.uint32).view(np.float32)


def denormal_tone_cases():
    """[(name, W, H, img)] for test_tone_and_gray8, no glare."""
    rng = np.random.default_rng(43)
    all_denormal = _from_bits(rng.permutation(np.arange(1, 36, dtype=np.uint32) * 3))
    wide = (2.0 ** np.linspace(-149, 127.9, 35)).astype(np.float32)
    max_flt = (rng.random(64 * 48, dtype=np.float32) * np.float32(3.0)).astype(np.float32)
    max_flt[1000], max_flt[2000] = FLT_MAX, TINY
    dz = _from_bits(rng.integers(1, 0x00800000, 35, dtype=np.uint32))
    dz[[0, 5, 11, 30]] = [-0.0, 0.0, 0.0, -0.0]
    dz[17] = _from_bits([0x007fffff])[0]
    # 34 dividends near 2^-110 under a maximum of 1.5 * 2^20: every quotient is
    # a subnormal of a few bits that the division has to round
    subq = (rng.random(35, dtype=np.float32) * np.float32(2.0 ** -110) + np.float32(2.0 ** -112)).astype(np.float32)
    subq[13] = np.float32(1.5 * 2.0 ** 20)
    # pixels 0..4 ulps below the maximum: tone's M - m is a few ulps of 1
    span = _from_bits(np.uint32(0x40000000) - (np.arange(35, dtype=np.uint32) * 3 + 4) % 5)
    return [("all_denormal", 7, 5, all_denormal), ("wide_range", 7, 5, wide), ("max_flt", 64, 48, max_flt),
            ("denormal_and_zero", 7, 5, dz), ("subnormal_quotients", 7, 5, subq), ("tiny_span", 7, 5, span)]


def is_subnormal(a):
    a = np.abs(np.asarray(a, np.float32))
    return (a > 0) & (a < TINY)


def check_denormal_tone_case(name, img, ref):
    """What makes each case of denormal_tone_cases non-trivial, on the CPU
    reference `ref` = display_ref(img). The subnormal counts also show that
    this process's float arithmetic does not flush them."""
    mx = dr.fold_max(img)
    with np.errstate(all="ignore"):
        q = (img / mx).astype(np.float32)
    tone = ref["tone"]
    if name == "all_denormal":
        assert is_subnormal(img).all() and len(np.unique(dr.bits(img))) == 35 and is_subnormal(mx)
        assert len(np.unique(dr.bits(tone))) == 35
    elif name == "wide_range":
        assert mx > FLT_MAX / 2 and is_subnormal(img[0]) and dr.bits(img)[0] == 1
        assert int((q < TINY).sum()) >= 10       # below the normal range: subnormal or rounded to zero
        assert int(is_subnormal(q).sum()) >= 3   # 2^e / mx for e in [-21.1, 1.9): three of the 35 exponents
        assert int(is_subnormal(q).sum()) + int((q == 0).sum()) == int((q < TINY).sum())
        assert int((tone > 0).sum()) >= 19       # powf's results are spread, not all zero
    elif name == "max_flt":
        assert mx == FLT_MAX and (img == TINY).sum() == 1
        assert int(is_subnormal(q).sum()) > 0.7 * img.size  # x / FLT_MAX is subnormal for x < 4
        assert len(np.unique(dr.bits(tone))) > 1000 and ref["gray8"].max() == 255
    elif name == "denormal_and_zero":
        assert is_subnormal(mx) and (is_subnormal(img) | (img == 0)).all()
        zb = dr.bits(img)[img == 0]
        assert (zb == 0).any() and (zb == 0x80000000).any()
        assert (tone[img == 0] == 0).all() and len(np.unique(ref["gray8"])) > 10
    elif name == "subnormal_quotients":
        assert mx == np.float32(1.5 * 2.0 ** 20) and int(is_subnormal(q).sum()) == 34
        exact = img.astype(np.float64) / float(mx)
        assert int((q[img != mx].astype(np.float64) != exact[img != mx]).sum()) >= 20  # inexact quotients
        assert len(np.unique(dr.bits(tone))) >= 30
    elif name == "tiny_span":
        assert dr.bits(mx).item() - int(dr.bits(img).min()) == 4 and len(np.unique(dr.bits(img))) == 5
        m, M = dr.fold_min(tone), dr.fold_max(tone)
        assert M == 1.0 and 1 <= dr.bits(M).item() - dr.bits(m).item() <= 4
        assert len(np.unique(ref["gray8"])) >= 2 and ref["gray8"].max() == 255 and ref["gray8"].min() == 0
    else:
        raise AssertionError(name)


# ---- D. two streams, one scratch -------------------------------------------
STREAM_CUTOFF = 50.0


@functools.lru_cache(maxsize=None)
def stream_cases():
    """{"L": (W, H, img), "S": (W, H, img)}: 256 x 256 with 2000 bright pixels
    and 64 x 48 with 40, at cutoff 50."""
    rng = np.random.default_rng(47)
    out = {}
    for key, W, H, k in (("L", 256, 256, 2000), ("S", 64, 48, 40)):
        img = dim(rng, W * H)
        hot = (rng.random(k, dtype=np.float32) * 40 + np.float32(51.5)).astype(np.float32)
        img[rng.choice(W * H, k, replace=False)] = hot
        img.setflags(write=False)
        out[key] = (W, H, img)
    return out


@functools.lru_cache(maxsize=None)
def stream_ref(key):
    W, H, img = stream_cases()[key]
    assert int((img > STREAM_CUTOFF).sum()) == {"L": 2000, "S": 40}[key]
    ref = dr.display_ref(img, W, H, STREAM_CUTOFF)
    if key == "L":  # unsaturated, so the order of the sums shows
        assert (ref["processed"] < STREAM_CUTOFF).sum() > 0.5 * W * H
    for v in ref.values():
        v.setflags(write=False)
    return ref
