"""The two-class kernels' hit / tie bookkeeping (csrc/optimize_lr_mfma.h),
restated in numpy.

lr_tie4 keeps min |u| as the minimum, in float32 order, of the values' high
words with the sign cleared, over a zero low word; the kernels only ever ask
`umin < 2^-52`.  lr_miss_add shifts the sign bit of each value's high word
into a 32-bit register (v_alignbit_b32 by 31) and lr_miss_count takes its
popcount; the one-step kernel counts and restarts the register before a group
of values that would not fit.
"""
import numpy as np

TIE = 2.0 ** -52
TIE_HI = 0x3CB00000


def _hi(u):
    return (np.asarray(u, np.float64).view(np.uint64) >> np.uint64(32)).astype(np.uint32)


def _hi_abs(u):
    return _hi(u) & np.uint32(0x7FFFFFFF)


def _prefilter(u, flush):
    """umin < 2^-52 as the kernel forms it: float32 minimum of the |high
    words| and 1.0's, rebuilt as the high word of a double.  `flush` models a
    float32 denormal flush of the minimum's inputs and result."""
    h = np.concatenate([_hi_abs(u).ravel(), np.array([0x3FF00000], np.uint32)])
    f = h.view(np.float32)
    assert np.all(np.isfinite(f))                 # |u| < 650: no NaN / inf pattern
    if flush:
        f = np.where(np.abs(f) < np.float32(2.0 ** -126), np.float32(0), f)
    m = np.float32(f.min())
    umin = (np.uint64(m.view(np.uint32)) << np.uint64(32)).view(np.float64)
    return bool(umin < TIE)


SPECIAL = [0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1040, 2.2250738585072014e-308, 2.0 ** -1015,
           2.0 ** -52, np.nextafter(2.0 ** -52, 0.0), np.nextafter(2.0 ** -52, 1.0),
           2.0 ** -53, 2.0 ** -40, 1.0, 160.0, 649.9]


def _values():
    rs = np.random.RandomState(0)
    mag = np.exp(rs.uniform(np.log(1e-300), np.log(650.0), 100000))
    rnd = mag * rs.choice([-1.0, 1.0], mag.size)
    sp = np.array(SPECIAL)
    return np.concatenate([sp, -sp, rnd])


def test_high_word_test_is_the_double_test():
    u = _values()
    assert np.array_equal(_hi_abs(u) < TIE_HI, np.abs(u) < TIE)
    # bit order of the |high words| is float32 order
    h = np.sort(_hi_abs(u))
    assert np.all(np.diff(h.view(np.float32).astype(np.float64)) >= 0)


def test_prefilter_one_value_at_a_time():
    for flush in (False, True):
        for x in _values()[:2 * len(SPECIAL) + 2000]:
            assert _prefilter(np.array([x]), flush) == (abs(x) < TIE), (x, flush)


def test_prefilter_over_groups():
    """Groups of 16 (a lane's values of four tiles): any value below 2^-52
    flags, none does not."""
    u = _values()
    big = u[np.abs(u) >= TIE]
    small = u[np.abs(u) < TIE]
    assert small.size > 10 and big.size > 1000
    rs = np.random.RandomState(1)
    for flush in (False, True):
        for _ in range(300):
            g = rs.choice(big, 16)
            assert not _prefilter(g, flush)
            g[rs.randint(16)] = rs.choice(small)
            assert _prefilter(g, flush)


def _alignbit(a, b, s):
    return np.uint32(((int(a) << 32 | int(b)) >> s) & 0xFFFFFFFF)


def _shift_count(u, valid, group):
    """Misses of the values u (padding rows, valid == False, always miss),
    taken `group` at a time as the one-step kernel's loop does: the register
    is counted and restarted before a group that would overflow its 32 bits."""
    miss, bits, missed = np.uint32(0), 0, 0
    for g0 in range(0, len(u), group):
        n = min(group, len(u) - g0)
        bits += n
        if bits > 32:
            missed += bin(int(miss)).count('1')
            miss, bits = np.uint32(0), n
        for x, v in zip(u[g0:g0 + n], valid[g0:g0 + n]):
            miss = _alignbit(miss, _hi(x) if v else 0x80000000, 31)
    return missed + bin(int(miss)).count('1')


def test_shift_register_count():
    rs = np.random.RandomState(2)
    pool = _values()
    for n in [1, 16, 32] + list(range(33, 41)):
        for group in (4, 8, 16):
            for rep in range(20):
                u = rs.choice(pool, n)
                valid = rs.rand(n) > 0.2 if rep % 2 else np.ones(n, bool)
                want = int(np.sum(np.signbit(u) | ~valid))
                assert _shift_count(u, valid, group) == want, (n, group)
    # every value a miss / none: the register exactly full
    assert _shift_count(-np.ones(32), np.ones(32, bool), 16) == 32
    assert _shift_count(np.ones(32), np.ones(32, bool), 16) == 0
    assert _shift_count(np.ones(40), np.zeros(40, bool), 4) == 40
