"""CosineDdf's quadrant from the draw (dropped): reduce_fast_
(ipt_math.h) finds the quadrant of phi = two_pi_times_u24(g) as
((int32)(phi * 0x1.45f306dc9c883p+23) + 2^23) >> 24, and the proposal was to
take it from the 24-bit draw as (g + 2^21) >> 22, without the f64 product and
its conversion. The two agree for every g but two, the draws that are exactly
2.5 and 3.5 quadrants: there phi rounds below the half-integer and
reduce_fast_ takes the lower quadrant. A sincosf_u24_ with the integer
quadrant would reduce those two angles by another multiple of pi/2 and is not
bit-exact, so it was not built; this test keeps the counterexamples.

The arithmetic is reduce_fast_'s own, restated in numpy: IEEE double products,
the rounding to float, a truncating conversion (every product is below 2^31).
"""
import struct

import numpy as np


def _d(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def test_quadrant_of_every_24_bit_draw():
    g = np.arange(1 << 24, dtype=np.uint64)
    phi = (_d(0x3E9921FB54442D18) * g.astype(np.float64)).astype(np.float32)  # two_pi_times_u24
    r = phi.astype(np.float64) * _d(0x41645F306DC9C883)                       # reduce_fast_: x * hpi_inv
    n_reduce = (r.astype(np.int32) + 0x800000) >> 24
    n_int = ((g + 0x200000) >> 22).astype(np.int32)
    bad = np.nonzero(n_reduce != n_int)[0]
    assert bad.tolist() == [0xA00000, 0xE00000]
    assert n_reduce[bad].tolist() == [2, 3] and n_int[bad].tolist() == [3, 4]
    # the other two half-integers round the other way and agree
    assert n_reduce[0x200000] == n_int[0x200000] == 1 and n_reduce[0x600000] == n_int[0x600000] == 2
    assert 0 <= n_reduce.min() and n_reduce.max() == 4
