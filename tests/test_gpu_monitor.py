"""The episode monitor's kernels (csrc/monitor_kernels.h) on synthetic rollout
records: torch tensors built from NumPy, no engine, so any done pattern is
reachable.  ``utils_logging.episodes_numpy`` / ``explained_variance_numpy`` are
the statements the kernels are held against.  The block scan runs at up to 8
count blocks in the first test and at 256, 257 and 261 in MANY_BLOCKS' tests
(more than one count per thread of its one workgroup)."""
import ctypes
import math

import numpy as np
import pytest

from custom_envs_amd import _native
from custom_envs_amd.utils import utils_logging as ul

pytestmark = pytest.mark.gpu

GUARD = 0xA5


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')


class Monitor:
    """A bare ce_monitor handle and one scan / write call."""

    def __init__(self, envs):
        self.lib = _native.load()
        self.envs = envs
        self.h = ctypes.c_void_p()
        _native.check(self.lib.ce_monitor_create(0, envs, ctypes.byref(self.h)), 'create')

    def close(self):
        self.lib.ce_monitor_destroy(self.h)

    def out_buffer(self, capacity, rb, guard=64):
        import torch
        return torch.full((capacity * rb + guard,), GUARD, dtype=torch.uint8, device='cuda')

    def scan(self, rec, cols, out, capacity):
        """Returns the total the scan reports."""
        import torch
        total = torch.full((1,), -7, dtype=torch.int64, device='cuda')
        k = rec['k']
        carr = (_native.CeMonitorColumn * max(1, len(cols)))()
        for j, c in enumerate(cols):
            carr[j] = _native.CeMonitorColumn(rec['info'].data_ptr(), rec['info'].stride(0) * 4,
                                              rec['info'].shape[2], c)
        _native.check(self.lib.ce_monitor_scan(
            self.h, k, self.envs, rec['P'], rec['reward'].data_ptr(), rec['reward'].stride(0) * 4,
            rec['done'].data_ptr(), rec['done'].stride(0), carr, len(cols), out.data_ptr(), capacity,
            total.data_ptr(), None), 'scan')
        torch.cuda.synchronize()
        return int(total.item())

    def write(self, out, capacity):
        import torch
        _native.check(self.lib.ce_monitor_write(self.h, out.data_ptr(), capacity, None), 'write')
        torch.cuda.synchronize()


def _records(K, E, P, rs, n_cols=9, pad=5, p_done=0.3, force=True, also=()):
    """Host arrays and their device records: reward / done [K][E * P] (an
    env's are its first agent row's; the other rows hold decoys) and info
    [K][E][n_cols], every record stride longer than the row.  ``also``: (t,
    env) pairs whose done is set whatever was drawn."""
    import torch
    reward = rs.normal(0, 3, (K, E * P)).astype(np.float32)
    done = (rs.rand(K, E * P) < p_done).astype(np.uint8)
    if force:
        done[K - 1, 0] = 1               # at least one finished episode
    for t, e in also:
        done[t, e * P] = 1
    info = rs.normal(0, 1, (K, E, n_cols)).astype(np.float32)

    def strided(a, extra):
        flat = a.reshape(K, -1)
        buf = np.full((K, flat.shape[1] + extra), 77, a.dtype)
        buf[:, :flat.shape[1]] = flat
        return torch.from_numpy(buf).cuda()[:, :flat.shape[1]]

    dev_info = torch.from_numpy(np.concatenate(
        [info.reshape(K, -1), np.full((K, pad), 77, np.float32)], axis=1)).cuda()
    dev_info = dev_info[:, :E * n_cols].unflatten(1, (E, n_cols))
    return {'k': K, 'P': P, 'reward': strided(reward, pad), 'done': strided(done, pad + 3),
            'info': dev_info, 'np': (reward[:, ::P], done[:, ::P], info)}


def _host(out, n, dtype):
    return out[:n * dtype.itemsize].cpu().numpy().view(dtype)


def _equal(got, want):
    assert len(got) == len(want)
    for name in want.dtype.names:        # field by field: the pad bytes are not compared
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert a.tobytes() == b.tobytes(), name


COLS = {0: (), 2: (7, 1), 7: (8, 0, 3, 2, 6, 4, 1)}


@pytest.mark.parametrize('E', [3, 65, 257])
@pytest.mark.parametrize('K', [1, 7])
@pytest.mark.parametrize('P', [1, 4])
@pytest.mark.parametrize('n_info', [0, 2, 7])
def test_records_equal_episodes_numpy(E, K, P, n_info):
    rs = np.random.RandomState(1000 * E + 10 * K + P + n_info)
    rec = _records(K, E, P, rs)
    reward, done, info = rec['np']
    cols = COLS[n_info]
    dtype = ul.record_dtype(n_info)
    want, carry = ul.episodes_numpy(reward, done, info[:, :, list(cols)] if cols else None)
    mon = Monitor(E)
    out = mon.out_buffer(K * E, dtype.itemsize)
    total = mon.scan(rec, cols, out, K * E)
    assert total == len(want)
    _equal(_host(out, total, dtype), want)
    # the carry the next call starts from
    state = ul.new_carry(E)
    _native.check(mon.lib.ce_monitor_get_state(
        mon.h, *(state[n].ctypes.data for n in ('ep_reward', 'ep_len', 'episode', 'total_steps')),
        None), 'get_state')
    for name in state:
        assert state[name].tobytes() == carry[name].tobytes(), name
    mon.close()


# The exclusive scan of the block counts (monitor_blockscan_kernel, one
# workgroup of 256 threads, thread i sums chunk = ceil(nb / 256) counts from
# i * chunk) beyond what the cases above reach (nb <= 8): nb = 256 is the last
# size with chunk = 1; nb = 257 has chunk = 2, the threads from 129 on with an
# empty range and thread 128 with a range clamped to one block; nb = 261 is
# the same with K > 1.  p_done = 0.02 keeps the records few.
MANY_BLOCKS = [(256, 256, 256), (1, 65537, 257), (65, 1025, 261)]


def _many_blocks(K, E, nb, seed):
    """Records with K * E flags in ``nb`` count blocks and a finished episode
    at the very last flag, at the first flag of block 256 and seven flags on
    (where they exist)."""
    n = K * E
    assert (n + 255) // 256 == nb
    flags = [i for i in (n - 1, 256 * 256, 256 * 256 + 7) if i < n]
    return _records(K, E, 1, np.random.RandomState(seed), p_done=0.02,
                    also=[divmod(i, E) for i in flags])


def _blocks_of(want, E):
    return (want['t'].astype(np.int64) * E + want['env']) // 256


@pytest.mark.parametrize('K,E,nb', MANY_BLOCKS)
@pytest.mark.parametrize('n_info', [0, 2])
def test_records_equal_episodes_numpy_beyond_256_count_blocks(K, E, nb, n_info):
    rec = _many_blocks(K, E, nb, 7 * nb + n_info)
    reward, done, info = rec['np']
    cols = COLS[n_info]
    dtype = ul.record_dtype(n_info)
    want, carry = ul.episodes_numpy(reward, done, info[:, :, list(cols)] if cols else None)
    blocks = _blocks_of(want, E)
    assert blocks.max() == nb - 1                    # a finished episode in the last count block
    if nb > 256:
        assert (blocks == 256).any()                 # and one past index 255
    assert len(np.unique(blocks)) > 200              # the offsets differ from block to block
    mon = Monitor(E)
    out = mon.out_buffer(len(want) + 8, dtype.itemsize)
    total = mon.scan(rec, cols, out, len(want) + 8)
    assert total == len(want)
    _equal(_host(out, total, dtype), want)
    assert (out[total * dtype.itemsize:].cpu().numpy() == GUARD).all()
    state = ul.new_carry(E)
    _native.check(mon.lib.ce_monitor_get_state(
        mon.h, *(state[n].ctypes.data for n in ('ep_reward', 'ep_len', 'episode', 'total_steps')),
        None), 'get_state')
    for name in state:
        assert state[name].tobytes() == carry[name].tobytes(), name
    mon.close()


def test_overflow_inside_a_count_block_past_255():
    """``capacity`` ends between two finished episodes of one count block
    past index 255: the first ``capacity`` records are written, the guard
    bytes after them are untouched, and ``ce_monitor_write`` delivers all."""
    K, E, nb = MANY_BLOCKS[2]
    cols = COLS[2]
    rec = _many_blocks(K, E, nb, 11)
    reward, done, info = rec['np']
    dtype = ul.record_dtype(2)
    rb = dtype.itemsize
    want, _ = ul.episodes_numpy(reward, done, info[:, :, list(cols)])
    blocks = _blocks_of(want, E)
    inside = [i for i in range(1, len(want)) if blocks[i] == blocks[i - 1] >= 256]
    assert inside
    capacity = inside[0]          # want[capacity - 1] and want[capacity]: one block past 255
    assert 0 < capacity < len(want)
    mon = Monitor(E)
    out = mon.out_buffer(capacity, rb, guard=4096)
    total = mon.scan(rec, cols, out, capacity)
    assert total == len(want)
    _equal(_host(out, capacity, dtype), want[:capacity])
    assert (out[capacity * rb:].cpu().numpy() == GUARD).all()
    big = mon.out_buffer(total, rb)
    mon.write(big, total)
    _equal(_host(big, total, dtype), want)
    assert (big[total * rb:].cpu().numpy() == GUARD).all()
    mon.close()


@pytest.mark.parametrize('E,P', [(65, 1), (257, 4)])
def test_two_calls_equal_one_call_on_the_concatenation(E, P):
    rs = np.random.RandomState(E)
    cols = COLS[2]
    dtype = ul.record_dtype(2)
    first, second = _records(7, E, P, rs, p_done=0.15), _records(7, E, P, rs, p_done=0.15)
    reward, done, info = (np.concatenate([a, b]) for a, b in zip(first['np'], second['np']))
    want, _ = ul.episodes_numpy(reward, done, info[:, :, list(cols)])
    assert (want['l'] > 7).any()             # an episode that spans the two calls
    mon = Monitor(E)
    got = []
    for part, t0 in ((first, 0), (second, 7)):
        out = mon.out_buffer(7 * E, dtype.itemsize)
        n = mon.scan(part, cols, out, 7 * E)
        rows = _host(out, n, dtype).copy()
        rows['t'] += t0
        got.append(rows)
    _equal(np.concatenate(got), want)
    mon.close()


def test_reset_and_set_state():
    E = 65
    rs = np.random.RandomState(5)
    rec = _records(7, E, 1, rs)
    reward, done, _ = rec['np']
    carry = ul.new_carry(E)
    carry['ep_reward'][:] = rs.normal(0, 1, E)
    carry['ep_len'][:] = rs.randint(0, 9, E)
    carry['episode'][:] = rs.randint(0, 5, E)
    carry['total_steps'][:] = 11
    mon = Monitor(E)
    _native.check(mon.lib.ce_monitor_set_state(
        mon.h, *(carry[n].ctypes.data for n in ('ep_reward', 'ep_len', 'episode', 'total_steps')),
        None), 'set_state')
    idx = np.array([0, 3, 3, 64], np.int32)              # a duplicate counts once
    _native.check(mon.lib.ce_monitor_reset(mon.h, idx.ctypes.data, idx.size, None), 'reset')
    for i in (0, 3, 64):
        carry['ep_reward'][i], carry['ep_len'][i] = 0.0, 0
        carry['episode'][i] += 1
    assert mon.lib.ce_monitor_reset(mon.h, np.array([65], np.int32).ctypes.data, 1,
                                    None) == _native.CE_EINVAL
    want, _ = ul.episodes_numpy(reward, done, None, carry)
    dtype = ul.record_dtype(0)
    out = mon.out_buffer(7 * E, dtype.itemsize)
    n = mon.scan(rec, (), out, 7 * E)
    _equal(_host(out, n, dtype), want)
    _native.check(mon.lib.ce_monitor_reset(mon.h, None, 0, None), 'reset all')
    state = ul.new_carry(E)
    _native.check(mon.lib.ce_monitor_get_state(
        mon.h, *(state[n].ctypes.data for n in ('ep_reward', 'ep_len', 'episode', 'total_steps')),
        None), 'get_state')
    assert not state['ep_reward'].any() and not state['ep_len'].any()
    assert (state['total_steps'] == 18).all()
    mon.close()


def test_overflow_reports_the_total_and_leaves_the_rest_untouched():
    E, K, cols = 257, 7, COLS[7]
    rs = np.random.RandomState(9)
    rec = _records(K, E, 4, rs)
    reward, done, info = rec['np']
    dtype = ul.record_dtype(7)
    rb = dtype.itemsize
    want, _ = ul.episodes_numpy(reward, done, info[:, :, list(cols)])
    mon = Monitor(E)
    assert mon.lib.ce_monitor_write(mon.h, None, 0, None) == _native.CE_ESTATE
    small = len(want) // 3
    assert 0 < small < len(want)
    out = mon.out_buffer(small, rb, guard=4096)
    total = mon.scan(rec, cols, out, small)
    assert total == len(want)                               # reported whatever the capacity
    _equal(_host(out, small, dtype), want[:small])
    assert (out[small * rb:].cpu().numpy() == GUARD).all()  # nothing past the capacity
    big = mon.out_buffer(total, rb)
    mon.write(big, total)                                   # the write alone, no second scan
    _equal(_host(big, total, dtype), want)
    assert (big[total * rb:].cpu().numpy() == GUARD).all()
    none = mon.out_buffer(0, rb)
    assert mon.scan(_records(1, E, 4, rs, p_done=0.0, force=False), cols, none, 0) == 0     # no done at all
    assert (none.cpu().numpy() == GUARD).all()
    mon.close()


def _ev(values, ret):
    import torch
    out = ul.explained_variance_device(values, ret)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_explained_variance():
    """|x| <= 10, Var[ret] >= 1e-3, n = 7 * 257 < 2^15 float32 terms summed in
    float64: each sum's relative error is at most n * 2^-53 ~ 2e-13, far inside
    the 1e-9 absolute bound."""
    import torch
    rs = np.random.RandomState(3)
    K, R, pad = 7, 257, 9
    ret = np.clip(rs.normal(0, 1, (K, R)), -10, 10).astype(np.float32)
    val = np.clip(ret + rs.normal(0, 1, (K, R)), -10, 10).astype(np.float32)
    assert np.var(ret.astype(np.float64)) >= 1e-3
    buf = np.full((K, R + pad), 1e6, np.float32)            # values strided in their records
    buf[:, :R] = val
    values = torch.from_numpy(buf).cuda()[:, :R]
    returns = torch.from_numpy(ret).cuda()
    got = _ev(values, returns)
    want = ul.explained_variance_numpy(val, ret)
    assert abs(float(got[0]) - want) <= 1e-9, (float(got[0]), want)
    assert _ev(values, returns).tobytes() == got.tobytes()  # bit-identical on a second run
    assert float(_ev(returns, returns)[0]) == 1.0
    const = torch.full((K, R), 2.5, dtype=torch.float32, device='cuda')
    assert math.isnan(float(_ev(values, const)[0]))         # Var[ret] == 0
    one = _ev(values[:1], returns[:1])                      # K = 1
    assert abs(float(one[0]) - ul.explained_variance_numpy(val[:1], ret[:1])) <= 1e-9
    # n = 3: 253 of the 256 threads hold no term; n = 256: one term each.
    # Fewer terms than above, so the same derivation and the same bound.
    for k, r in ((1, 3), (1, 256), (2, 128)):
        assert np.var(ret[:k, :r].astype(np.float64)) >= 1e-3
        few = _ev(values[:k, :r], returns[:k, :r].contiguous())
        want = ul.explained_variance_numpy(val[:k, :r], ret[:k, :r])
        assert abs(float(few[0]) - want) <= 1e-9, (k, r, float(few[0]), want)
