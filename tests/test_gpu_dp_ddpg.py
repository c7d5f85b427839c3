"""DDPG's side of the gradient exchange on the device, in one process: one
agent plays the W ranks in turn -- ``partial`` per shard into slot r of one
records tensor, then ``combine`` / ``apply`` -- so no collective and no second
process are involved (tests/test_gpu_dp_learn_ranks.py has those).

1. Global gradient parity: ``combine`` of the ranks' records against
   ``ddpg_cases.reference`` on the whole case, held to test_gpu_ddpg.py's
   ``_check`` (1e-5 per block, 1e-5 on the statistics): CASES[2] as array
   shards [33, 32, 5], CASES[4] as ``idx`` slices [1, 129] of one permutation,
   SHAPE_CASES[0] as [33, 32].  The record's tail holds n_r and zeros.
2. World 1 is today's step: ``partial`` + ``apply`` of one shard leaves
   parameters, targets, Adam's state and statistics bit-equal to ``step`` on a
   twin, three steps, once with ``actor_lr=0``; ``train`` with a world-1
   exchange (``collective=False``) is bit-equal to ``train`` without one.
3. Three steps of shards [33, 32, 5] follow ``train_step_numpy`` within the
   bound test_gpu_ddpg.py holds ``step`` to.
4. The same shards twice give the same bits; another rank order stays within
   the bound.
5. The weight is global: records formed with ``n_total = n_r`` miss the bound.
"""
import numpy as np
import pytest

import ddpg_cases as cases
import test_gpu_ddpg as td
from custom_envs_amd import _native, ddpg, learner as base
from custom_envs_amd.ddpg import ReplayMemory
from custom_envs_amd.rng import DeviceRng

pytestmark = pytest.mark.gpu

BOUND = td.BOUND
SPLITS = [(cases.CASES[2], [33, 32, 5], 'array'), (cases.CASES[4], [1, 129], 'idx'),
          (cases.SHAPE_CASES[0], [33, 32], 'array')]
_np, _cuda = td._np, td._cuda


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')


def _bounds(shards):
    edges = np.concatenate([[0], np.cumsum(shards)])
    return [slice(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]


def _shards(inputs, shards, mode):
    """[(batch, idx)] per rank: contiguous arrays of their own, or ``idx``
    slices of one fixed permutation of the whole batch."""
    assert sum(shards) == inputs['obs0'].shape[0]
    if mode == 'array':
        return [({n: _cuda(inputs[n][s]) for n in cases.FIELDS}, None) for s in _bounds(shards)]
    whole = td._dev(inputs)
    perm = _cuda(np.random.RandomState(3).permutation(sum(shards)).astype(np.int32))
    return [(whole, perm[s]) for s in _bounds(shards)]


def _records(agent, parts, n_total=None, order=None):
    """The ranks' records, rank r from parts[order[r]]; ``n_total`` None: each
    shard's own row count (the wrong weight)."""
    import torch
    order = list(range(len(parts))) if order is None else order
    records = torch.zeros((len(parts), agent.record_doubles), dtype=torch.float64, device='cuda')
    for r, i in enumerate(order):
        batch, idx = parts[i]
        agent.partial(batch, idx, n_total=n_total, out=records[r])
    return records


def _state(agent):
    opt = agent.get_opt_state()
    return [agent.get_params(), agent.get_params(target=True), opt['m'], opt['v'],
            np.array(opt['step'])]


# --------------------------------------------------------- 1. gradient parity
@pytest.mark.parametrize('case, shards, mode', SPLITS, ids=str)
def test_global_gradient_parity(case, shards, mode):
    import torch
    agent, inputs = td._agent(case)
    assert _native.load().ce_ddpg_record_bytes(agent._h) == agent.record_doubles * 8
    records = _records(agent, _shards(inputs, shards, mode), case[0])
    grad, stats = agent.combine(records, case[0])
    torch.cuda.synchronize()
    tail = _np(records)[:, agent.n_params:]
    assert np.array_equal(tail[:, 2 * base.ROW_STATS], shards)
    assert not tail[:, 2 * base.ROW_STATS + 1:].any()
    td._check(case, _np(grad), stats, cases.reference(case), 'dp ddpg %s' % shards)
    # the statement of partial + combine, from the device's own records
    assert np.array_equal(_np(grad), ddpg.combine_records_numpy(_np(records), agent.n_params,
                                                                np.float32))
    agent.close()


# ----------------------------------------------------- 2. world 1 is today's
@pytest.mark.parametrize('case, mode', [(cases.CASES[2], 'array'), (cases.CASES[4], 'idx')], ids=str)
def test_world_1_partial_apply_is_step(case, mode):
    dp, inputs = td._agent(case, tau=0.01)
    twin, _ = td._agent(case, tau=0.01)
    (batch, idx), = _shards(inputs, [case[0]], mode)
    for t, lrs in enumerate([{}, dict(actor_lr=0.0), dict(actor_lr=2e-4, critic_lr=5e-4)]):
        records = _records(dp, [(batch, idx)], case[0])
        s_dp = dp.apply(records, case[0], **lrs)
        s_one = twin.step(batch, idx, **lrs)
        for a, b in zip(_state(dp), _state(twin)):
            assert np.array_equal(a, b), t
        assert np.array_equal(_np(s_dp.tensor), _np(s_one.tensor)), t
    assert not np.array_equal(dp.get_params(), inputs['params'])
    dp.close(), twin.close()


def _memory_of(inputs):
    N, D = inputs['obs0'].shape
    memory = ReplayMemory(N, N, D, inputs['actions'].shape[1])
    for n in cases.FIELDS:
        getattr(memory, n).copy_(_cuda(inputs[n]))
    memory.advance()
    assert memory.size == N
    return memory


def test_world_1_train_under_an_exchange_is_train():
    import torch
    from custom_envs_amd.distributed import GradientExchange
    case = cases.CASES[2]
    dp, inputs = td._agent(case, tau=0.01)
    twin, _ = td._agent(case, tau=0.01)
    ex = GradientExchange(dp, 0, 1, collective=False)
    assert dp.exchange is ex and twin.exchange is None and ex.moments is None
    memory = _memory_of(inputs)
    g_dp, g_one = DeviceRng(11), DeviceRng(11)
    for steps in (3, 2):
        s_dp = dp.train(memory, steps, 48, g_dp)
        s_one = twin.train(memory, steps, 48, g_one)
        torch.cuda.synchronize()
        assert np.array_equal(_np(s_dp), _np(s_one))
        assert g_dp.replay_t == g_one.replay_t
        for a, b in zip(_state(dp), _state(twin)):
            assert np.array_equal(a, b)
    # step and grad go the same way
    batch = td._dev(inputs)
    assert np.array_equal(_np(dp.step(batch).tensor), _np(twin.step(batch).tensor))
    g0, s0 = dp.grad(batch)
    g1, s1 = twin.grad(batch)
    assert np.array_equal(_np(g0), _np(g1)) and np.array_equal(_np(s0.tensor), _np(s1.tensor))
    assert np.array_equal(_np(s0.y), _np(s1.y))
    dp.close(), twin.close()


# ------------------------------------------- 3. sharded steps, the statement
def test_three_sharded_steps_follow_the_statement():
    case = cases.CASES[2]
    hyper = dict(tau=0.01, actor_lr=1e-4, critic_lr=1e-3)
    agent, inputs = td._agent(case, **hyper)
    N, D, hidden, A, _ = case
    parts = _shards(inputs, [33, 32, 5], 'array')
    p = inputs['params'].astype(np.float64)
    tp = inputs['target_params'].astype(np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    host = cases.batch_of(inputs)
    for t in (1, 2, 3):
        before_t = agent.get_params(target=True)
        stats = agent.apply(_records(agent, parts, N), N)
        p, tp, m, v, ref_stats = ddpg.train_step_numpy(p, tp, m, v, t, host, agent.n_actor,
                                                       hp=cases.HP, hidden=hidden, **hyper)
        got_p, got_t = agent.get_params(), agent.get_params(target=True)
        ep, et = cases.rel_err(got_p, p), cases.rel_err(got_t, tp)
        serr = td._stat_errs(stats.stats(), ref_stats)
        print('dp step', t, 'params %.3g targets %.3g' % (ep, et), serr)
        assert ep <= BOUND and et <= BOUND
        assert max(serr.values()) <= BOUND
        assert np.array_equal(got_t, ddpg.soft_update_numpy(before_t, got_p, hyper['tau']))
    assert agent.get_opt_state()['step'] == 3
    agent.close()


# ------------------------------------------------- 4. determinism and order
def test_same_shards_twice_and_another_rank_order():
    case = cases.CASES[2]
    agent, inputs = td._agent(case)
    parts = _shards(inputs, [33, 32, 5], 'array')
    first = _records(agent, parts, case[0])
    g0, s0 = agent.combine(first, case[0])
    second = _records(agent, parts, case[0])
    g1, s1 = agent.combine(second, case[0])
    assert np.array_equal(_np(first), _np(second))
    assert np.array_equal(_np(g0), _np(g1)) and np.array_equal(_np(s0.tensor), _np(s1.tensor))
    g2, s2 = agent.combine(_records(agent, parts, case[0], order=[2, 0, 1]), case[0])
    td._check(case, _np(g2), s2, cases.reference(case), 'dp ddpg order 2 0 1')
    agent.close()


# ------------------------------------------------------ 5. the global weight
def test_each_shards_own_weight_misses_the_bound():
    case = cases.CASES[2]
    agent, inputs = td._agent(case)
    parts = _shards(inputs, [33, 32, 5], 'array')
    ref = cases.reference(case)[1]
    right, _ = agent.combine(_records(agent, parts, case[0]), case[0])
    wrong, _ = agent.combine(_records(agent, parts, None), case[0])
    e_right = max(cases.block_errs(case, _np(right), ref).values())
    e_wrong = max(cases.block_errs(case, _np(wrong), ref).values())
    print('global weight %.3g, each shard its own %.3g' % (e_right, e_wrong))
    assert e_right <= BOUND < e_wrong
    agent.close()
