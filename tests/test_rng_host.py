"""The counter-based generator's NumPy statement (custom_envs_amd/rng.py) and
the argument checks of its C entries.  No test here needs a GPU."""
import ctypes

import numpy as np
import pytest

from custom_envs_amd import _native, rng

KNOWN = [
    ((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     'd16cfe09 94fdcceb 5001e420 24126ea1'),
]


@pytest.mark.parametrize('counter,key,want', KNOWN)
def test_philox_known_answers(counter, key, want):
    got = rng.philox_numpy(counter, key)
    assert ' '.join('%08x' % int(w) for w in got) == want


def test_philox_vectorised_equals_elementwise():
    rs = np.random.RandomState(0)
    c = rs.randint(0, 2 ** 32, (4, 3, 5), dtype=np.uint64).astype(np.uint32)
    k = rs.randint(0, 2 ** 32, (2, 3, 5), dtype=np.uint64).astype(np.uint32)
    whole = rng.philox_numpy(tuple(c), tuple(k))
    assert all(w.dtype == np.uint32 and w.shape == (3, 5) for w in whole)
    for i in range(3):
        for j in range(5):
            one = rng.philox_numpy(tuple(c[:, i, j]), tuple(k[:, i, j]))
            assert [int(w) for w in one] == [int(w[i, j]) for w in whole]
    # broadcasting a scalar key and counter words over an array
    rows = np.arange(7, dtype=np.uint32)
    b = rng.philox_numpy((rows, 3, 0, 1), (5, 6))
    for r in range(7):
        assert [int(w[r]) for w in b] == [int(w) for w in rng.philox_numpy((r, 3, 0, 1), (5, 6))]


def test_uniform_is_strictly_inside_the_unit_interval():
    x = np.array([0, 1, 255, 256, 0x7fffffff, 0x80000000, 0xffffff00, 0xffffffff], np.uint32)
    u = rng.uniform_numpy(x)
    assert u.dtype == np.float64
    assert np.all(u > 0.0) and np.all(u < 1.0)
    assert u[0] == 2.0 ** -25 and u[-1] == 1.0 - 2.0 ** -25
    # the largest |z|: r at the smallest u
    assert np.sqrt(-2.0 * np.log(u[0])) <= rng.MAX_ABS_NORMAL


def test_normal_columns_do_not_depend_on_act_dim():
    a3 = rng.normal_numpy(77, 5, 9, 3)
    a20 = rng.normal_numpy(77, 5, 9, 20)
    assert a3.shape == (9, 3) and a20.shape == (9, 20) and a3.dtype == np.float64
    assert np.array_equal(a3, a20[:, :3])
    assert np.array_equal(rng.normal_numpy(77, 5, 9, 4), a20[:, :4])
    assert not np.array_equal(a20, rng.normal_numpy(77, 6, 9, 20))          # another draw
    assert not np.array_equal(a20, rng.normal_numpy(78, 5, 9, 20))          # another seed
    assert not np.array_equal(a20, rng.normal_numpy(77 + 2 ** 32, 5, 9, 20))  # the high word counts
    assert not np.array_equal(a20, rng.normal_numpy(77, 5, 9, 20, purpose=rng.PREDICT))
    assert rng.normal_numpy(77, 5, 9, 20, dtype=np.float32).dtype == np.float32


def test_normal_row_offset_is_the_global_row():
    whole = rng.normal_numpy(3, 2, 40, 5)
    for off in (1, 7, 33):
        part = rng.normal_numpy(3, 2, 40 - off, 5, row_offset=off)
        assert np.array_equal(part, whole[off:])


def test_normal_moments():
    z = np.stack([rng.normal_numpy(1234, t, 4096, 16) for t in range(64)])
    assert z.size == 4194304
    mean, std, worst = float(z.mean()), float(z.std()), float(np.abs(z).max())
    print('normal moments: mean %.3e std %.6f max %.3f' % (mean, std, worst))
    assert abs(mean) < 2e-3
    assert abs(std - 1.0) < 2e-3
    assert worst <= 5.89


def test_u32_stream_layout():
    u = rng.u32_numpy(9, rng.PERMUTATION, 4, 10)
    assert u.dtype == np.uint32 and u.shape == (10,)
    for i in range(10):
        words = rng.philox_numpy((0, 4, i // 4, rng.PERMUTATION), (9, 0))
        assert int(u[i]) == int(words[i % 4])
    assert np.array_equal(rng.u32_numpy(9, rng.PERMUTATION, 4, 7), u[:7])


def test_permutation_is_a_permutation_and_differs_between_epochs():
    for n in (1, 5, 64, 1000):
        p = rng.permutation_numpy(11, 0, n)
        assert p.dtype == np.int32 and sorted(p.tolist()) == list(range(n))
    assert not np.array_equal(rng.permutation_numpy(11, 0, 64), rng.permutation_numpy(11, 1, 64))
    keys = rng.u32_numpy(11, rng.PERMUTATION, 0, 64)
    assert np.array_equal(rng.permutation_numpy(11, 0, 64), np.argsort(keys, kind='stable'))


def test_device_rng_bookkeeping_without_a_device():
    g = rng.DeviceRng(2 ** 40 + 5, device=None, row_offset=3)
    assert (g.t, g.epoch) == (0, 0)
    g.advance(10)
    g.t += 2
    assert g.t == 12
    state = g.state()
    assert all(isinstance(v, int) for v in state.values())
    h = rng.DeviceRng(0, device=None)
    h.set_state(state)
    assert h.state() == state
    g.t = 2 ** 32 - 4
    g.check_draws(4)
    with pytest.raises(ValueError):
        g.check_draws(5)
    with pytest.raises(ValueError):
        g.advance(5)
    with pytest.raises(ValueError):
        rng.DeviceRng(-1, device=None)
    with pytest.raises(ValueError):
        rng.DeviceRng(2 ** 64, device=None)
    with pytest.raises(RuntimeError):
        g.normal(1, 2, 3)


# ------------------------------------------------------------- the C entries
def _einval(rc, *words):
    assert rc == _native.CE_EINVAL
    msg = _native.load().ce_last_error().decode()
    for w in words:
        assert w in msg, msg


def test_rng_normal_argument_checks():
    lib = _native.load()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    _einval(lib.ce_rng_normal(None, 1, 1, 1, 4, 0, 0, 0, None), 'ce_rng_normal', 'null')
    _einval(lib.ce_rng_normal(p, 0, 1, 1, 4, 0, 0, 0, None), 'k must')
    _einval(lib.ce_rng_normal(p, 1, 0, 1, 4, 0, 0, 0, None), 'rows')
    _einval(lib.ce_rng_normal(p, 1, -3, 1, 4, 0, 0, 0, None), 'rows')
    _einval(lib.ce_rng_normal(p, 1, 1, 0, 4, 0, 0, 0, None), 'act_dim')
    _einval(lib.ce_rng_normal(p, 1, 1, 65, 260, 0, 0, 0, None), 'act_dim')
    _einval(lib.ce_rng_normal(p, 2, 2, 3, 20, 0, 0, 0, None), 'record_stride_bytes')
    _einval(lib.ce_rng_normal(p, 2, 1, 1, 4, 0, 2 ** 32 - 1, 0, None), '2^32')
    _einval(lib.ce_rng_normal(p, 1, 2, 1, 8, 0, 0, 2 ** 32 - 1, None), '2^32')


def test_rng_u32_argument_checks():
    lib = _native.load()
    buf = np.zeros(8, np.uint32)
    _einval(lib.ce_rng_u32(None, 4, 0, 1, 0, None), 'ce_rng_u32', 'null')
    _einval(lib.ce_rng_u32(buf.ctypes.data, 0, 0, 1, 0, None), 'n must')
    _einval(lib.ce_rng_u32(buf.ctypes.data, 2 ** 31 + 1, 0, 1, 0, None), 'n must')


def test_policy_rng_entries_argument_checks():
    lib = _native.load()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    po = _native.CePolicyOutputs(action=p, env_action=p, neglogp=p, value=p)
    eo, mo = _native.CeOutputs(), _native.CeMultiOutputs()
    _einval(lib.ce_policy_forward_rng(None, p, 0, 0, 0, 1, ctypes.byref(po), None), 'null')
    _einval(lib.ce_policy_forward_rng(p, None, 0, 0, 0, 1, ctypes.byref(po), None), 'null')
    # a non-null policy is never dereferenced before these fail
    _einval(lib.ce_policy_forward_rng(p, p, 0, 0, 0, 0, ctypes.byref(po), None), 'rows')
    _einval(lib.ce_policy_forward_rng(p, p, 0, 0, 0, 1, ctypes.byref(_native.CePolicyOutputs()),
                                      None), 'outputs')
    _einval(lib.ce_policy_forward_rng(p, p, 0, 0, 2 ** 32 - 1, 2, ctypes.byref(po), None), '2^32')
    for fn, out in ((lib.ce_rollout_policy_rng, eo), (lib.ce_multi_rollout_policy_rng, mo)):
        _einval(fn(None, None, 1, p, 0, 0, 0, ctypes.byref(out), 0, ctypes.byref(po), 0), 'null')
        # t0 + k > 2^32 is refused before the engine is looked at
        _einval(fn(None, None, 2, p, 0, 2 ** 32 - 1, 0, ctypes.byref(out), 0, ctypes.byref(po), 0),
                '2^32')


def test_opt_state_entries_argument_checks():
    lib = _native.load()
    buf = np.zeros(8, np.float32)
    p = buf.ctypes.data
    step = ctypes.c_int64(0)
    for pre in ('ce_ppo2', 'ce_a2c'):
        get, put = getattr(lib, pre + '_get_opt_state'), getattr(lib, pre + '_set_opt_state')
        _einval(get(None, p, p, 8, ctypes.byref(step), 0, None), 'null learner')
        _einval(get(None, None, p, 8, ctypes.byref(step), 0, None), 'null')
        _einval(get(None, p, p, 8, None, 0, None), 'null step')
        _einval(put(None, p, p, 8, 0, 0, None), 'null learner')
        _einval(put(None, p, None, 8, 0, 0, None), 'null')
    _einval(lib.ce_ppo2_set_opt_state(None, p, p, 8, -1, 0, None), 'step')
    _einval(lib.ce_a2c_set_opt_state(None, p, p, 8, 3, 0, None), 'step')


def test_header_exports_and_ctypes_table_agree():
    import os
    import re
    from conftest import ROOT
    lib = _native.load()
    assert lib.ce_abi_version() == 5 == _native.ABI_VERSION
    text = open(os.path.join(ROOT, 'include', 'custom_envs_amd.h')).read()
    declared = set(re.findall(r'^\s*(?:const\s+)?\w+\s+\**\s*(ce_\w+)\s*\(', text, re.M))
    new = {'ce_rng_normal', 'ce_rng_u32', 'ce_policy_forward_rng', 'ce_rollout_policy_rng',
           'ce_multi_rollout_policy_rng', 'ce_ppo2_get_opt_state', 'ce_ppo2_set_opt_state',
           'ce_a2c_get_opt_state', 'ce_a2c_set_opt_state'}
    assert new <= declared and new <= set(_native.EXPORTS)
    assert declared == set(_native.EXPORTS)
    for name in new:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name
    # the argument counts of the table against the header's declarations
    flat = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in new:
        args = re.search(r'\b%s\s*\(([^)]*)\)' % name, flat).group(1)
        assert len(getattr(lib, name).argtypes) == len(args.split(',')), name
