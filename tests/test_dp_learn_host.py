"""Data-parallel ``learn`` and DDPG's side of the gradient exchange, without a
GPU.

1. ``ddpg.combine_records_numpy``: shards [33, 32, 5] of ddpg_cases.CASES[2],
   each ``loss_grad_numpy`` gradient weighted n_r / N, against the whole case
   (1e-12); the statistic sums fold to the whole case's statistics.
2. ``rng.permutation_numpy`` / ``replay_indices_numpy`` with ``offset`` /
   ``total``: world 1 is the short call bit for bit, the ranks' slices are
   disjoint parts of one stream, every result is a permutation / in range.
3. ``distribute`` on shape-only models: ``row_offset``, the global ``n_batch``
   and ``check_learn``, DDPG's "train this cycle" decision for uneven counts,
   every refusal.
4. The record layout follows ``n_params`` on a shape-only ``DDPGAgent``; the
   ``ValueError``s that precede any native call; the new entry points refuse
   bad arguments without a device.
"""
import ctypes

import numpy as np
import pytest

import ddpg_cases as cases
from custom_envs_amd import _native, agents, ddpg, learner as base, rng
from custom_envs_amd.agents import A2C, DDPG, PPO2, EnvSpec, MlpPolicy
from custom_envs_amd.ddpg import DDPGAgent

CASE = cases.CASES[2]                 # 70 rows, D = 41, hidden (64, 64), A = 20
SHARDS = [33, 32, 5]


def _bounds(shards):
    edges = np.concatenate([[0], np.cumsum(shards)])
    return [slice(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]


# ------------------------------------------------------------------ 1. combine
def shard_records(case, shards):
    """(records [W][record], the whole case's (stats, grad)) in float64."""
    inputs = cases.draw_case(case)
    N, hidden = case[0], case[2]
    records = []
    for s in _bounds(shards):
        n_r = s.stop - s.start
        st, g = ddpg.loss_grad_numpy(inputs['params'], inputs['target_params'],
                                     *[inputs[f][s] for f in cases.FIELDS], hp=cases.HP,
                                     hidden=hidden)
        sums = np.zeros(2 * base.ROW_STATS)
        sums[0], sums[1], sums[2] = (st['critic_loss'] * n_r, st['q_mean'] * n_r,
                                     st['target_mean'] * n_r)
        sums[base.ROW_STATS] = -st['actor_loss'] * n_r
        records.append(base.pack_record_numpy(g * n_r / N, sums, n_r))
    return np.stack(records), cases.reference(case)


def test_combined_ddpg_records_are_the_whole_batch_gradient():
    records, (ref_stats, whole) = shard_records(CASE, SHARDS)
    n = whole.size
    assert records.shape == (3, base.record_doubles(n)) and records.shape[1] * 8 % 256 == 0
    assert np.array_equal(records[:, n + 2 * base.ROW_STATS], SHARDS)
    assert np.all(records[:, n + 2 * base.ROW_STATS + 1:] == 0.0)
    got = ddpg.combine_records_numpy(records, n)
    err = np.max(np.abs(got - whole))
    print('combine', SHARDS, err)
    assert err <= 1e-12
    # a shard's own mean (n_total = n_r) is not the global weight
    unweighted = records[:, :n] * (CASE[0] / np.asarray(SHARDS, np.float64))[:, None]
    assert np.max(np.abs(unweighted.sum(axis=0) - whole)) > 1e-3
    g32 = ddpg.combine_records_numpy(records, n, np.float32)
    assert g32.dtype == np.float32 and np.array_equal(g32, got.astype(np.float32))
    sums = records[:, n:n + 2 * base.ROW_STATS].sum(axis=0) / CASE[0]
    assert abs(sums[0] - ref_stats['critic_loss']) <= 1e-12 * abs(ref_stats['critic_loss'])
    assert abs(-sums[base.ROW_STATS] - ref_stats['actor_loss']) <= 1e-12
    assert abs(sums[1] - ref_stats['q_mean']) <= 1e-12 and abs(sums[2] - ref_stats['target_mean']) <= 1e-12


# ------------------------------------------------------------------- 2. streams
@pytest.mark.parametrize('counts, K', [([4, 2], 4), ([33, 32, 5], 2), ([7], 3)], ids=str)
def test_rank_permutations_use_disjoint_slices_of_one_key_stream(counts, K):
    seed, t = 2 ** 40 + 17, 5
    total = K * sum(counts)
    keys = rng.u32_numpy(seed, rng.PERMUTATION, t, total)
    off = 0
    for c in counts:
        n = K * c
        perm = rng.permutation_numpy(seed, t, n, offset=K * off, total=total)
        assert perm.dtype == np.int32 and np.array_equal(np.sort(perm), np.arange(n))
        assert np.array_equal(perm, np.argsort(keys[K * off:K * off + n], kind='stable'))
        # a word does not depend on the stream's length
        assert np.array_equal(perm, rng.permutation_numpy(seed, t, n, offset=K * off))
        off += c
    assert K * off == total                # the slices tile the stream: disjoint keys
    assert np.array_equal(rng.permutation_numpy(seed, t, total, offset=0, total=total),
                          rng.permutation_numpy(seed, t, total))


def test_rank_replay_indices_map_their_columns_onto_their_own_memory():
    seed, t, B = 99, 3, 6
    sizes = [48, 12, 7]
    W = len(sizes)
    words = rng.u32_numpy(seed, rng.REPLAY, t, W * B).astype(np.uint64)
    for r, size in enumerate(sizes):
        idx = rng.replay_indices_numpy(seed, t, B, size, offset=r * B, total=W * B)
        assert idx.dtype == np.int32 and idx.min() >= 0 and idx.max() < size
        assert np.array_equal(idx, ((words[r * B:(r + 1) * B] * np.uint64(size)) >> np.uint64(32))
                              .astype(np.int32))
    assert np.array_equal(rng.replay_indices_numpy(seed, t, B, 48, offset=0, total=B),
                          rng.replay_indices_numpy(seed, t, B, 48))
    for bad in (dict(offset=-1), dict(offset=3, total=8), dict(offset=0, total=5)):
        with pytest.raises(ValueError, match='slice'):
            rng.replay_indices_numpy(seed, t, B, 48, **bad)
        with pytest.raises(ValueError, match='slice'):
            rng.permutation_numpy(seed, t, B, **bad)


# ---------------------------------------------------------------- 3. distribute
def _spec(rows):
    return EnvSpec(rows, 6, 2, low=-0.5, high=0.5, device=None)


KW = dict(policy_kwargs=dict(net_arch=[dict(pi=[32], vf=[32])]), seed=3)


@pytest.mark.parametrize('algo', ['ppo2', 'a2c'])
def test_distribute_sets_the_row_offset_and_counts_timesteps_globally(algo):
    counts = [4, 2]
    for rank in (0, 1):
        if algo == 'ppo2':
            model = PPO2(MlpPolicy, _spec(counts[rank]), n_steps=4, nminibatches=2, **KW)
        else:
            model = A2C(MlpPolicy, _spec(counts[rank]), n_steps=3, **KW)
        k = model.n_steps
        assert model.n_batch == counts[rank] * k and model.rng.row_offset == 0
        ex = model.distribute(rank, 2, counts=counts, collective=False, broadcast=False)
        assert model.learner.exchange is ex and ex.counts == counts and not ex.collective
        assert model.rng.row_offset == sum(counts[:rank])
        assert model.n_batch == 6 * k
        assert model.check_learn(2 * 6 * k + 1) == 2          # the same on every rank
        with pytest.raises(ValueError, match='less than one batch'):
            model.check_learn(6 * k - 1)
        with pytest.raises(RuntimeError, match='already'):
            model.distribute(rank, 2, counts=counts, collective=False, broadcast=False)


def test_distribute_refusals_precede_everything():
    def model(rows=4, **kw):
        return PPO2(MlpPolicy, _spec(rows), n_steps=4, nminibatches=2, **dict(KW, **kw))

    with pytest.raises(ValueError, match='shape-only'):
        model().distribute(0, 2, counts=[4, 2], collective=False)
    with pytest.raises(ValueError, match='counts says 3 rows, the env has 4'):
        model().distribute(0, 2, counts=[3, 2], collective=False, broadcast=False)
    with pytest.raises(ValueError, match='bad rank/world'):
        model().distribute(2, 2, collective=False, broadcast=False)
    with pytest.raises(ValueError, match='every one of the 2 ranks'):
        model().distribute(0, 2, counts=[4], collective=False, broadcast=False)
    # rank 1's 3 * 3 rows do not split in two: rank 0 refuses as well
    m = PPO2(MlpPolicy, _spec(4), n_steps=3, nminibatches=2, **KW)
    with pytest.raises(ValueError, match='rank 1: .* 9 rows do not split into 2'):
        m.distribute(0, 2, counts=[4, 3], collective=False, broadcast=False)
    assert m.dist is None and m.learner.exchange is None and m.rng.row_offset == 0
    # default counts: this env's rows on every rank
    m = model()
    m.distribute(1, 3, collective=False, broadcast=False)
    assert m.dist.counts == [4, 4, 4] and m.rng.row_offset == 4 and m.n_batch == 48


def _ddpg(rows, **kw):
    args = dict(nb_rollout_steps=3, nb_train_steps=2, batch_size=8, buffer_size=48, seed=5,
                policy_kwargs=dict(layers=[32]))
    args.update(kw)
    return DDPG(ddpg.MlpPolicy, _spec(rows), **args)


def test_ddpg_ranks_skip_and_train_together():
    """[4, 2] rows, 3 rollout steps, batch 8: rank 0 holds 12 records after the
    first cycle, rank 1 only 6, so the first cycle trains on neither."""
    counts = [4, 2]
    decisions = []
    for rank in (0, 1):
        model = _ddpg(counts[rank])
        ex = model.distribute(rank, 2, counts=counts, collective=False, broadcast=False)
        assert model.agent.exchange is ex and ex.moments is None
        assert ex.counts == [1, 1] and ex.total_rows(8) == 16     # equal batch shares
        assert model.rng.row_offset == sum(counts[:rank])
        assert model.n_batch == 6 * 3 and model.check_learn(3 * 18) == 3
        decisions.append([model.trains_after(c) for c in (1, 2, 3)])
    assert decisions[0] == decisions[1] == [False, True, True]
    assert agents.ddpg_ranks_ready(counts, [0, 0], [48, 48], 1, 3, 8) is False
    assert agents.ddpg_ranks_ready(counts, [0, 6], [48, 48], 1, 3, 8) is True
    # a ring never holds more than its capacity
    assert agents.ddpg_ranks_ready([4, 2], [0, 0], [48, 6], 9, 3, 8) is False


def test_ddpg_distribute_refusals():
    with pytest.raises(ValueError, match='shape-only'):
        _ddpg(4).distribute(0, 2, counts=[4, 2], collective=False)
    with pytest.raises(ValueError, match='counts says 2 rows, the env has 4'):
        _ddpg(4).distribute(0, 2, counts=[2, 4], collective=False, broadcast=False)
    # rank 1's ring (buffer_size rounded down to a multiple of 5 rows) is below batch_size
    with pytest.raises(ValueError, match='rank 1: buffer_size rounds down to 5'):
        _ddpg(4, buffer_size=8).distribute(0, 2, counts=[4, 5], collective=False, broadcast=False)
    noise = ddpg.OrnsteinUhlenbeckActionNoise(np.zeros(2), 0.1 * np.ones(2))
    noise.set_state(np.zeros((3, 2), np.float32), np.zeros(3, np.uint8))
    m = _ddpg(4, action_noise=noise)
    with pytest.raises(ValueError, match='Ornstein-Uhlenbeck state holds 3 rows'):
        m.distribute(0, 2, counts=[4, 2], collective=False, broadcast=False)
    assert m.dist is None and m.agent.exchange is None
    m = _ddpg(4)
    m.distribute(0, 2, counts=[4, 2], collective=False, broadcast=False)
    with pytest.raises(RuntimeError, match='already'):
        m.distribute(0, 2, counts=[4, 2], collective=False, broadcast=False)


# -------------------------------------------------------- 4. records, C checks
def _cpu_batch(M=6, D=5, A=2):
    import torch
    return {'obs0': torch.zeros(M, D), 'actions': torch.zeros(M, A), 'rewards': torch.zeros(M),
            'obs1': torch.zeros(M, D), 'dones': torch.zeros(M, dtype=torch.uint8)}


@pytest.mark.parametrize('shape', [(5, 2, (32,)), (41, 20, (64, 64)), (128, 33, (32, 64))], ids=str)
def test_record_layout_follows_n_params(shape):
    D, A, hidden = shape
    agent = DDPGAgent(D, A, hidden, device=None)
    rd = agent.record_doubles
    assert rd == base.record_doubles(agent.n_params) and rd * 8 % 256 == 0
    assert agent.n_params + base.RECORD_TAIL <= rd < agent.n_params + base.RECORD_TAIL + 32
    assert agent.exchange is None


def test_shape_only_agent_checks_precede_any_native_call():
    import torch
    from custom_envs_amd.distributed import GradientExchange
    agent = DDPGAgent(5, 2, (32,), device=None)
    rd = agent.record_doubles
    with pytest.raises(ValueError, match='n_total = 5 is less than the 6 rows'):
        agent.partial(_cpu_batch(), n_total=5)
    with pytest.raises(ValueError, match='shape'):
        agent.partial(_cpu_batch(), out=torch.zeros(rd + 32, dtype=torch.float64))
    with pytest.raises(ValueError, match='float64'):
        agent.partial(_cpu_batch(), out=torch.zeros(rd, dtype=torch.float32))
    with pytest.raises(ValueError, match='y must have shape'):
        agent.partial(_cpu_batch(), y=torch.zeros(5))
    for call in (lambda r: agent.apply(r, n_total=8), lambda r: agent.combine(r, n_total=8)):
        with pytest.raises(ValueError, match='float64'):
            call(torch.zeros(2, rd, dtype=torch.float32))
        with pytest.raises(ValueError, match='shape'):
            call(torch.zeros(2, rd - 32, dtype=torch.float64))
        with pytest.raises(ValueError, match='shape'):
            call(torch.zeros(2 * rd, dtype=torch.float64))
        with pytest.raises(ValueError, match='n_total'):
            agent.apply(torch.zeros(2, rd, dtype=torch.float64), n_total=0)
    with pytest.raises(ValueError, match='actor_lr'):
        agent.apply(torch.zeros(1, rd, dtype=torch.float64), n_total=8, actor_lr=-1.0)
    with pytest.raises(_native.NativeEngineError, match='shape-only'):
        agent.partial(_cpu_batch())
    ex = GradientExchange(agent, 1, 3)
    assert agent.exchange is ex and ex.moments is None and ex.records.device.type == 'cpu'
    assert tuple(ex.records.shape) == (3, rd) and ex.bytes_per_step == 3 * rd * 8
    assert ex.total_rows(128) == 3 * 128
    ex.detach()
    assert agent.exchange is None


def _refused(rc, word):
    msg = _native.load().ce_last_error().decode()
    assert rc == _native.CE_EINVAL, (rc, msg)
    assert word in msg, msg


def test_new_entry_points_are_exported_and_refuse_bad_arguments():
    lib = _native.load()
    for name in ('ce_ddpg_record_bytes', 'ce_ddpg_partial', 'ce_ddpg_combine', 'ce_ddpg_apply'):
        assert name in _native.EXPORTS and hasattr(lib, name), name
    assert lib.ce_abi_version() == 5
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data
    assert lib.ce_ddpg_record_bytes(None) == -1
    assert b'null learner' in lib.ce_last_error()

    def partial(n=4, n_total=4, m=4, idx=None, record=p, y=p, handle=None):
        return lib.ce_ddpg_partial(handle, n, n_total, m, idx, p, p, p, p, p, y, record, None)

    _refused(partial(n=0), 'n must be at least 1')
    _refused(partial(n=5), 'n exceeds m')
    _refused(partial(n_total=3), 'n_total must be in [n, 2^30]')
    _refused(partial(n_total=2 ** 30 + 1), 'n_total must be in [n, 2^30]')
    _refused(partial(record=None), 'null record')
    _refused(partial(record=p + 4), '8-byte aligned')
    _refused(partial(y=None), 'null y buffer')
    _refused(partial(), 'null learner')
    for fn, tail in ((lib.ce_ddpg_combine, (p, p, None)), (lib.ce_ddpg_apply, (-1.0, -1.0, p, None))):
        _refused(fn(None, 0, p, 8, *tail), 'world must be in [1, 2^16]')
        _refused(fn(None, 2, p, 0, *tail), 'n_total must be in [1, 2^30]')
        _refused(fn(None, 2, None, 8, *tail), 'null records')
        _refused(fn(None, 2, p + 4, 8, *tail), '8-byte aligned')
        _refused(fn(None, 2, p, 8, *tail), 'null learner')
    _refused(lib.ce_ddpg_combine(None, 2, p, 8, None, p, None), 'null grad')
    _refused(lib.ce_ddpg_combine(None, 2, p, 8, p, None, None), 'null stats')
    _refused(lib.ce_ddpg_apply(None, 2, p, 8, float('nan'), -1.0, p, None), 'not a number')
    _refused(lib.ce_ddpg_apply(None, 2, p, 8, -1.0, -1.0, None, None), 'null stats')
    assert ctypes.sizeof(ctypes.c_double) == 8
