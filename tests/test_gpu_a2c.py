"""The A2C learner on the device (ce_a2c_*, csrc/a2c_kernels.h) against the
NumPy statements of custom_envs_amd/a2c.py in float64.

1. Returns parity on true strided rollout records (K = 5, episodes of 4 steps,
   R = 1, 3, 65 envs of the two-class shape and the 8 agent rows of func4):
   1e-5 norm-relative against ``returns_numpy`` in float64, and bit-equal to
   ``returns_numpy`` in float32 (the kernel keeps its multiplies and adds
   unfused and in the statement's order).
2. Gradient parity, the inputs of every case of ppo2_cases (CASES and the
   unequal and 96-wide SHAPE_CASES): each parameter block within 1e-5 of
   ``loss_grad_numpy`` in float64 (max|d| / max|ref over the whole gradient|);
   each network (pi, vf, logstd) within max(1e-5, 2 x the float32 NumPy
   statement's own error) of it in max|d| / max|ref over that network|
   (``ppo2_cases.net_errs``); each statistic and ``grad_norm`` within 1e-5
   relative.
3. ``idx``: a shuffled subset of a larger batch equals the contiguous call on
   the gathered copy bit for bit; a permutation of all rows stays in the bound.
4. In place equals flat: ``update(result)`` and ``step(flatten(result,
   returns(result)))`` of a real ``collect`` leave bit-identical parameters and
   statistics, both within 1e-5 of the float64 statement.
5. Determinism (the same call twice, bit-identical) and grid independence
   (grid_limit 1, 2, 0 agree to the bound).
6. Three ``step`` calls against ``loss_grad_numpy`` + ``rmsprop_step_numpy`` in
   float64, the norm clip biting and idle; the policy image follows.
7. collect -> update -> collect, and its bit-identical replay.
"""
import numpy as np
import pytest

import policy_cases as pc
import ppo2_cases as cases
from custom_envs_amd.a2c import (STAT_NAMES, A2CLearner, HyperParams, loss_grad_numpy,
                                 returns_numpy, rmsprop_step_numpy)
from custom_envs_amd.policy import MlpPolicy, dict_to_flat, forward_numpy

pytestmark = pytest.mark.gpu

BOUND = 1e-5
HP = HyperParams(0.01, 0.25)
FIELDS = ('obs', 'actions', 'returns', 'values')
K = 5


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')


def _np(t):
    return t.detach().cpu().numpy()


def _dev(inputs):
    import torch
    return {n: torch.from_numpy(np.ascontiguousarray(inputs[n])).cuda() for n in FIELDS}


def _learner(case, grid_limit=None, **over):
    inputs = cases.inputs_of(case)
    _, D, hidden, A, limit = case
    policy = MlpPolicy(D, A, hidden)
    hyper = dict(ent_coef=HP.ent_coef, vf_coef=HP.vf_coef,
                 grid_limit=limit if grid_limit is None else grid_limit)
    hyper.update(over)
    learner = A2CLearner(policy, **hyper)
    learner.set_params(inputs['params'])
    return learner, inputs


_REF, _REF32 = {}, {}


def _reference(case):
    """(stats, grad) of the float64 statement, computed once per case."""
    if case not in _REF:
        inputs = cases.inputs_of(case)
        _REF[case] = loss_grad_numpy(inputs['params'], *[inputs[n] for n in FIELDS], hp=HP,
                                     hidden=inputs['hidden'])
    return _REF[case]


def _statement32(case):
    """The float32 statement's gradient on the case's inputs, computed once."""
    if case not in _REF32:
        inputs = cases.inputs_of(case)
        _REF32[case] = loss_grad_numpy(inputs['params'], *[inputs[n] for n in FIELDS], hp=HP,
                                       hidden=inputs['hidden'], dtype=np.float32)[1]
    return _REF32[case]


def _stat_errs(got, ref_stats):
    return {n: abs(got[n] - float(ref_stats[n])) / abs(float(ref_stats[n]))
            if float(ref_stats[n]) != 0.0 else abs(got[n]) for n in STAT_NAMES}


def _check(case, grad, stats, ref, what, g32=None):
    """``g32``: the float32 statement's gradient on the inputs ``ref`` was
    computed from; the case's own when ``ref`` is ``_reference(case)``."""
    ref_stats, ref_grad = ref
    if g32 is None:
        assert ref is _REF.get(case), 'a reference of other inputs needs its own float32 statement'
        g32 = _statement32(case)
    nerrs, nbounds = cases.net_errs(case, grad, ref_grad), cases.net_bounds(case, g32, ref_grad)
    print(what, case, 'per network', nerrs, 'bounds', nbounds)
    errs = cases.block_errs(case, grad, ref_grad)
    got = stats.stats()
    serr = _stat_errs(got, ref_stats)
    ref_norm = float(np.sqrt(np.sum(np.asarray(ref_grad) ** 2)))
    nerr = abs(got['grad_norm'] - ref_norm) / ref_norm
    print(what, case, 'worst block %.3g' % max(errs.values()), errs, serr, 'grad_norm %.3g' % nerr)
    for name, err in errs.items():
        assert err <= BOUND, (what, name, err)
    for net, err in nerrs.items():
        assert err <= nbounds[net], (what, net, err, nbounds[net])
    for name, err in serr.items():
        assert err <= BOUND, (what, name, err)
    assert nerr <= BOUND, what
    host = _np(stats.tensor)
    assert host[4] == 0.0 and host[5] == 0.0 and host[7] == 0.0


# --------------------------------------------------------------- 1. returns
def _rollout(name, num_envs, stream_handle):
    """A K-step closed-loop rollout of `num_envs` envs of a policy_cases
    shape on the given stream: (engine, policy, env fields, policy fields,
    last_values, rows)."""
    import torch
    kind, kw = pc.ROLLOUT_SHAPES[name]
    rows, D, A = pc.rollout_dims(name)
    if kind == 'optimize':
        from custom_envs_amd.engine import OptimizeEngine
        features, targets = pc.rollout_dataset(name)
        eng = OptimizeEngine(features, targets, num_envs=num_envs, batch_size=kw['batch_size'],
                             max_steps=4)
        eng.seed([21 + i for i in range(num_envs)])
        rows = num_envs
    else:
        from custom_envs_amd.multi_engine import MultiOptEngine
        eng = MultiOptEngine(num_envs, kw['problem'], max_batches=4, max_history=5)
        rows = num_envs * (rows // kw['num_envs'])
    eng.set_stream(stream_handle)
    params, _ = pc.rollout_policy_inputs(name)
    policy = MlpPolicy(D, A, pc.ROLLOUT_HIDDEN)
    policy.set_params(params)
    noise = np.random.RandomState(11).normal(0, 1, (K, rows, A)).astype(np.float32)
    first = eng.alloc_device_outputs()
    eng.reset_device(first)
    fields, rec, pfields, prec = eng.alloc_policy_rollout(K, policy)
    eng.rollout_policy(K, policy, first['obs'], torch.from_numpy(noise).cuda(), fields, rec,
                       pfields, prec)
    last = policy.forward_device(fields['obs'][K - 1])
    return eng, policy, fields, pfields, last['value'], rows


@pytest.mark.parametrize('name, num_envs', [('lr_two_class_f64', 1), ('lr_two_class_f64', 3),
                                            ('lr_two_class_f64', 65), ('multi_func4', 2)])
def test_returns_parity_on_rollout_records(name, num_envs):
    import torch
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):       # the engine's launches and the learner's share it
        eng, policy, fields, pfields, last_values, rows = _rollout(name, num_envs,
                                                                   stream.cuda_stream)
        learner = A2CLearner(policy, gamma=0.99)
        rewards, dones = fields['reward'], fields['done']
        assert tuple(rewards.shape) == (K, rows) and tuple(dones.shape) == (K, rows)
        # strided records: the stride exceeds a record
        assert rewards.stride(0) > rows and dones.stride(0) > rows
        ret = learner.returns(rewards=rewards, dones=dones, last_values=last_values)
        stream.synchronize()
    r, d, lv = _np(rewards), _np(dones), _np(last_values)
    assert np.array_equal((d != 0).sum(axis=0), np.ones(rows))      # one episode end per row
    assert tuple(ret.shape) == (K, rows) and ret.is_contiguous()
    ref = returns_numpy(r, d, lv, 0.99)
    err = np.linalg.norm(_np(ret) - ref) / np.linalg.norm(ref)
    print('returns', name, rows, err)
    assert err <= BOUND
    assert np.array_equal(_np(ret), returns_numpy(r, d, lv, 0.99, dtype=np.float32))
    learner.close()
    policy.close()
    eng.close()


# ---------------------------------------------------------- 2. gradient parity
@pytest.mark.parametrize('case', cases.CASES + cases.SHAPE_CASES,
                         ids=cases.CASE_IDS + cases.SHAPE_CASE_IDS)
def test_gradient_parity(case):
    import torch
    learner, inputs = _learner(case)
    grad, stats = learner.grad(_dev(inputs))
    torch.cuda.synchronize()
    _check(case, _np(grad), stats, _reference(case), 'gradient parity')
    # the statement in float32 on the same inputs, for scale
    print('float32 statement', case,
          max(cases.block_errs(case, _statement32(case), _reference(case)[1]).values()))
    learner.close()
    learner.policy.close()


# ------------------------------------------------------------------- 3. idx
def test_idx_gathers_rows():
    _idx_gathers_rows(cases.CASES[3], 70)        # 130 rows


def test_idx_gathers_rows_of_shrink_then_grow_widths():
    _idx_gathers_rows(cases.SHAPE_CASES[3], 33)  # (128, 32, 64), A = 32: 33 of 40 rows


def _idx_gathers_rows(case, n_sub):
    import torch
    learner, inputs = _learner(case)
    batch = _dev(inputs)
    rs = np.random.RandomState(7)
    sub = rs.permutation(case[0])[:n_sub].astype(np.int32)
    gathered = {n: inputs[n][sub] for n in FIELDS}
    args = [gathered[n] for n in FIELDS]
    ref = loss_grad_numpy(inputs['params'], *args, hp=HP, hidden=inputs['hidden'])
    _, g32 = loss_grad_numpy(inputs['params'], *args, hp=HP, hidden=inputs['hidden'],
                             dtype=np.float32)
    g_idx, s_idx = learner.grad(batch, torch.from_numpy(sub).cuda())
    g_copy, s_copy = learner.grad(_dev(gathered))
    torch.cuda.synchronize()
    _check(case, _np(g_idx), s_idx, ref, 'idx subset', g32)
    _check(case, _np(g_copy), s_copy, ref, 'gathered copy', g32)
    assert np.array_equal(_np(g_idx), _np(g_copy))       # the same rows in the same order
    assert np.array_equal(_np(s_idx.tensor), _np(s_copy.tensor))
    # every row, permuted: the summation order alone differs
    perm = rs.permutation(case[0]).astype(np.int32)
    g_perm, s_perm = learner.grad(batch, torch.from_numpy(perm).cuda())
    torch.cuda.synchronize()
    _check(case, _np(g_perm), s_perm, _reference(case), 'idx permutation')
    learner.close()
    learner.policy.close()


# ------------------------------------------------------ 4. in place equals flat
def _collect_env(name, num_envs):
    """(env, obs_dim, act_dim, rows, params) of a K-step collect shape."""
    import functools
    rows, D, A = pc.rollout_dims(name)
    params, _ = pc.rollout_policy_inputs(name)
    if pc.ROLLOUT_SHAPES[name][0] == 'optimize':
        from custom_envs_amd.vectorize.gpuvecenv import GPUVecEnv
        features, targets = pc.rollout_dataset(name)
        env = GPUVecEnv(num_envs, data_set=(features, targets), max_steps=4,
                        seed=[21 + i for i in range(num_envs)])
        return env, D, A, num_envs, params
    from custom_envs_amd.envs.multioptlrs import MultiOptLRs
    from custom_envs_amd.vectorize.optvecenv import OptVecEnv
    problem = pc.ROLLOUT_SHAPES[name][1]['problem']
    env = OptVecEnv([functools.partial(MultiOptLRs, problem=problem, max_batches=4)
                     for _ in range(num_envs)])
    assert env.engine_backed
    return env, D, A, num_envs * (rows // pc.ROLLOUT_SHAPES[name][1]['num_envs']), params


@pytest.mark.parametrize('name, num_envs, rows', [('lr_two_class_f64', 3, 3),
                                                  ('lr_two_class_f64', 65, 65),
                                                  ('multi_func4', 2, 8)])
def test_update_in_place_equals_flat_step(name, num_envs, rows):
    import torch
    env, D, A, got_rows, params = _collect_env(name, num_envs)
    assert got_rows == rows
    flat0 = dict_to_flat(params, MlpPolicy(D, A, pc.ROLLOUT_HIDDEN, device=None).params_layout())
    lr = 0.1             # one large step: the parity bound below resolves it to 10 % or better
    learners = []
    for _ in range(2):
        policy = MlpPolicy(D, A, pc.ROLLOUT_HIDDEN)
        policy.set_params(params)
        learners.append(A2CLearner(policy, lr=lr))
    in_place, flat = learners
    noise = torch.from_numpy(np.random.RandomState(17).normal(0, 1, (K, rows, A))
                             .astype(np.float32)).cuda()
    env.reset()
    result = env.collect(in_place.policy, K, noise)
    # the policy records are strided, the observations contiguous
    assert result['actions'].stride(0) > rows * A and result['values'].stride(0) > rows
    assert not result['actions'].is_contiguous() and result['obs'].is_contiguous()
    ret = flat.returns(result)
    batch = flat.flatten(result, ret)
    assert tuple(batch['obs'].shape) == (K * rows, D)
    s_flat = flat.step(batch)
    s_in = in_place.update(result)
    torch.cuda.synchronize()
    p_in, p_flat = in_place.get_params(), flat.get_params()
    assert np.array_equal(p_in, p_flat)
    assert np.array_equal(_np(s_in.tensor), _np(s_flat.tensor))
    # the float64 statement on the same rollout
    host = {n: _np(batch[n]) for n in FIELDS}
    ref_ret = returns_numpy(_np(result['rewards']), _np(result['dones']),
                            _np(result['last_values']), 0.99)
    assert np.linalg.norm(host['returns'] - ref_ret.reshape(-1)) <= BOUND * np.linalg.norm(ref_ret)
    ref_stats, g = loss_grad_numpy(flat0, host['obs'], host['actions'], ref_ret.reshape(-1),
                                   host['values'], hp=HyperParams(0.01, 0.25),
                                   hidden=pc.ROLLOUT_HIDDEN)
    p, _, _ = rmsprop_step_numpy(flat0.astype(np.float64), g, np.ones_like(g), np.zeros_like(g),
                                 lr, 0.5)
    perr = np.linalg.norm(p_in - p) / np.linalg.norm(p)
    got = s_in.stats()
    serr = _stat_errs(got, ref_stats)
    ref_norm = float(np.sqrt(np.sum(g * g)))
    nerr = abs(got['grad_norm'] - ref_norm) / ref_norm
    print('in place', name, rows, 'params %.3g' % perr, serr, 'grad_norm %.3g' % nerr)
    assert perr <= BOUND
    moved = np.linalg.norm(p - flat0) / np.linalg.norm(p)
    print('in place', name, rows, 'moved %.3g' % moved)
    assert moved > 10 * BOUND
    for n, err in serr.items():
        assert err <= BOUND, (n, err)
    assert nerr <= BOUND
    env.close()
    for learner in learners:
        learner.close()
        learner.policy.close()


# ------------------------------------------- 5. determinism, grid independence
# with the 96 -> 96 row and the three unequal layers
TWICE_CASES = [cases.CASES[2], cases.CASES[4], cases.SHAPE_CASES[4], cases.SHAPE_CASES[2]]
TWICE_IDS = [cases.CASE_IDS[2], cases.CASE_IDS[4], cases.SHAPE_CASE_IDS[4], cases.SHAPE_CASE_IDS[2]]


@pytest.mark.parametrize('case', TWICE_CASES, ids=TWICE_IDS)
def test_same_call_twice_is_bit_identical(case):
    import torch
    learner, inputs = _learner(case)
    batch = _dev(inputs)
    g1, s1 = learner.grad(batch)
    g2, s2 = learner.grad(batch)
    torch.cuda.synchronize()
    assert np.array_equal(_np(g1), _np(g2))
    assert np.array_equal(_np(s1.tensor), _np(s2.tensor))
    learner.close()
    learner.policy.close()


@pytest.mark.parametrize('case', TWICE_CASES, ids=TWICE_IDS)
def test_grid_limits_agree(case):
    import torch
    grads = {}
    for limit in (1, 2, 0):
        learner, inputs = _learner(case, grid_limit=limit)
        grad, stats = learner.grad(_dev(inputs))
        torch.cuda.synchronize()
        grads[limit] = _np(grad)
        _check(case, grads[limit], stats, _reference(case), 'grid_limit %d' % limit)
        learner.close()
        learner.policy.close()
    for limit in (2, 0):
        errs = cases.block_errs(case, grads[limit], grads[1].astype(np.float64))
        assert max(errs.values()) <= BOUND, (limit, errs)


# ------------------------------------------------------------------ 6. step
# lr: a clipped RMSProp step from ms = 1 is lr * max_grad_norm long, so the
# clipped run takes the larger rate to move the parameters visibly
@pytest.mark.parametrize('case, max_grad_norm, bites, lr', [(cases.CASES[2], 0.05, True, 0.2),
                                                            (cases.CASES[3], 100.0, False, 1e-2),
                                                            (cases.SHAPE_CASES[1], 0.05, True, 0.2)],
                         ids=['clip_bites', 'clip_idle', 'clip_bites_h32x128'])
def test_three_steps_follow_the_statement(case, max_grad_norm, bites, lr):
    import torch
    learner, inputs = _learner(case, max_grad_norm=max_grad_norm, lr=lr)
    batch = _dev(inputs)
    args = [inputs[n] for n in FIELDS]
    p = inputs['params'].astype(np.float64)
    ms, mom = np.ones_like(p), np.zeros_like(p)
    for t in (1, 2, 3):
        ref_stats, g = loss_grad_numpy(p, *args, hp=HP, hidden=inputs['hidden'])
        assert (np.sqrt(np.sum(g * g)) > max_grad_norm) == bites
        p, ms, mom = rmsprop_step_numpy(p, g, ms, mom, lr, max_grad_norm)
        stats = learner.step(batch)
        got = learner.get_params()
        err = np.linalg.norm(got - p) / np.linalg.norm(p)
        print('step', t, case, err, stats.stats()['loss'], float(ref_stats['loss']))
        assert err <= BOUND, (t, err)
        assert abs(stats.stats()['loss'] - float(ref_stats['loss'])) <= BOUND * abs(float(ref_stats['loss']))
    assert np.linalg.norm(p - inputs['params']) > 100 * BOUND * np.linalg.norm(p)    # it moved
    # the policy's image was repacked: its forward is the statement's at p
    out = learner.policy.forward_device(batch['obs'])
    torch.cuda.synchronize()
    ref = forward_numpy(inputs['obs'], None, p, inputs['hidden'])
    assert pc.rel_err(_np(out['action']), ref['mean']) <= BOUND
    assert pc.rel_err(_np(out['value']), ref['value']) <= BOUND
    learner.close()
    learner.policy.close()


# ----------------------------------------------------------- 7. closed loop
def _closed_loop():
    import torch
    from custom_envs_amd.vectorize.gpuvecenv import GPUVecEnv
    name, E = 'lr_two_class_f64', 3
    features, targets = pc.rollout_dataset(name)
    rows, D, A = pc.rollout_dims(name)
    params, _ = pc.rollout_policy_inputs(name)
    policy = MlpPolicy(D, A, pc.ROLLOUT_HIDDEN)
    policy.set_params(params)
    learner = A2CLearner(policy, lr=1e-2)
    noise = torch.from_numpy(np.random.RandomState(13).normal(0, 1, (2, K, rows, A))
                             .astype(np.float32)).cuda()
    env = GPUVecEnv(E, data_set=(features, targets), max_steps=4, seed=[21, 22, 23])
    env.reset()
    first = env.collect(policy, K, noise[0])
    stats = learner.update(first)
    second = env.collect(policy, K, noise[1])
    torch.cuda.synchronize()
    out = {'values0': _np(first['values']), 'values1': _np(second['values']),
           'rewards1': _np(second['rewards']), 'params': learner.get_params(),
           'stats': _np(stats.tensor)}
    env.close()
    learner.close()
    policy.close()
    return out


def test_collect_update_collect():
    a = _closed_loop()
    assert a['stats'].shape == (8,)
    for key in a:
        assert np.isfinite(a[key]).all(), key
    assert not np.array_equal(a['values0'], a['values1'])
    # the first value of the second rollout comes from the updated network
    assert np.max(np.abs(a['values1'][0] - a['values0'][-1])) > 0
    b = _closed_loop()
    for key in a:
        assert np.array_equal(a[key], b[key]), key
