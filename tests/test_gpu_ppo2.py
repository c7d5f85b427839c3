"""The PPO2 learner on the device (ce_ppo2_*, csrc/ppo2_kernels.h) against the
NumPy statements of custom_envs_amd/ppo2.py in float64.

1. GAE parity on true strided rollout records (K = 10, episodes of 4 steps,
   R = 1, 3, 65 envs of the two-class shape and the 8 agent rows of func4):
   1e-5 norm-relative against ``gae_numpy`` in float64, and bit-equal to
   ``gae_numpy`` in float32 (the kernel keeps its multiplies and adds unfused
   and in the statement's order).
2. Gradient parity, every case of ppo2_cases (CASES and the unequal and
   96-wide SHAPE_CASES): each parameter block within 1e-5 of
   ``loss_grad_numpy`` in float64 (max|d| / max|ref over the whole gradient|);
   each network (pi, vf, logstd) within max(1e-5, 2 x the float32 NumPy
   statement's own error) of it in max|d| / max|ref over that network|
   (``ppo2_cases.net_errs``: the value network's gradient is 4 to 25 times
   smaller than the policy's, which the first measure hides); each statistic
   within 1e-5 relative (a pg_loss that cancels within 1e-5 of the mean size
   of its terms, see ``_check``), clipfrac exact.
3. ``idx``: a shuffled subset of a larger batch equals the contiguous call on
   the gathered copy; a permutation of all rows differs by summation order.
4. Determinism: the same call twice, bit-identical.
5. Grid independence: grid_limit 1, 2, 0 agree to the bound.
6. Three ``step`` calls against ``loss_grad_numpy`` + ``adam_step_numpy`` in
   float64, the norm clip biting and idle; the policy image follows.
7. collect -> gae -> update -> collect, and its bit-identical replay.
8. The whole ``update`` on consistent synthetic rollouts with explicit
   permutations: bit-identical to the hand-written gae -> flatten -> step
   loop, and against ``ppo2_cases.update_numpy`` in float64 (the bounds and
   the measured values are in the test's docstring).
"""
import numpy as np
import pytest

import policy_cases as pc
import ppo2_cases as cases
from custom_envs_amd.policy import MlpPolicy, forward_numpy
from custom_envs_amd.ppo2 import (STAT_NAMES, PPO2Learner, adam_step_numpy, gae_numpy,
                                  loss_grad_numpy)

pytestmark = pytest.mark.gpu

BOUND = 1e-5


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')


def _np(t):
    return t.detach().cpu().numpy()


def _dev(inputs, names=cases.BATCH_FIELDS):
    import torch
    return {n: torch.from_numpy(np.ascontiguousarray(inputs[n])).cuda() for n in names}


def _learner(case, grid_limit=None, **over):
    inputs = cases.inputs_of(case)
    _, D, hidden, A, limit = case
    policy = MlpPolicy(D, A, hidden)
    hyper = dict(cliprange=cases.HP.cliprange, cliprange_vf=cases.HP.cliprange_vf,
                 ent_coef=cases.HP.ent_coef, vf_coef=cases.HP.vf_coef,
                 normalize_adv=cases.HP.normalize_adv,
                 grid_limit=limit if grid_limit is None else grid_limit)
    hyper.update(over)
    learner = PPO2Learner(policy, **hyper)
    learner.set_params(inputs['params'])
    return learner, inputs


_REF, _SIDE = {}, {}


def _reference(case):
    """(stats, grad) of the float64 statement, computed once per case."""
    if case not in _REF:
        inputs = cases.inputs_of(case)
        _REF[case] = loss_grad_numpy(inputs['params'], *[inputs[n] for n in cases.BATCH_FIELDS],
                                     hp=cases.HP, hidden=inputs['hidden'])
    return _REF[case]


def _side(inputs, hp):
    """What the bounds of ``_check`` are taken from, on the CPU: the float32
    statement's gradient and the float64 terms of pg_loss on ``inputs``."""
    _, g32 = loss_grad_numpy(inputs['params'], *[inputs[n] for n in cases.BATCH_FIELDS], hp=hp,
                             hidden=inputs['hidden'], dtype=np.float32)
    return g32, cases.pg_terms(inputs, hp)


def _statement32(case):
    """``_side`` of the case's own inputs, computed once."""
    if case not in _SIDE:
        _SIDE[case] = _side(cases.inputs_of(case), cases.HP)
    return _SIDE[case]


def _check(case, grad, stats, ref, what, inputs=None, hp=cases.HP):
    """``inputs``, ``hp``: what ``ref`` was computed from, when that is not
    the case's own draw under ``cases.HP`` (``ref`` is then ``_reference(case)``).

    Every statistic is held to 1e-5 relative to itself.  The one exception is
    a pg_loss that cancels: where its condition number mean|term| / |mean|
    exceeds ``cases.PG_COND_MAX`` (see ``cases.pg_terms``; 185 to 351 on three
    of the SHAPE_CASES, 3 to 46 on every other input of these tests) 1e-5 of
    the mean is less than a tenth of a float32 rounding of one term, and
    pg_loss is held to 1e-5 of mean|term| instead, the project's float32 bound
    on the scale of what is summed.  That scaled bound is asserted on every
    call; on CASES the condition number is asserted to be below the limit, so
    the relative assertion cannot lapse there."""
    ref_stats, ref_grad = ref
    if inputs is None:
        assert ref is _REF.get(case), 'a reference of other inputs needs those inputs'
        g32, terms = _statement32(case)
    else:
        g32, terms = _side(inputs, hp)
    nerrs, nbounds = cases.net_errs(case, grad, ref_grad), cases.net_bounds(case, g32, ref_grad)
    print(what, case, 'per network', nerrs, 'bounds', nbounds)
    errs = cases.block_errs(case, grad, ref_grad)
    got = stats.stats()
    serr, pg_cond, pg_scaled = _stat_errs(got, ref_stats, terms)
    print(what, case, 'worst block %.3g' % max(errs.values()), errs, serr,
          'pg_loss: condition %.1f, |d| / mean|term| %.3g' % (pg_cond, pg_scaled))
    if case in cases.CASES:
        assert pg_cond <= cases.PG_COND_MAX, (what, pg_cond)
    for name, err in errs.items():
        assert err <= BOUND, (what, name, err)
    for net, err in nerrs.items():
        assert err <= nbounds[net], (what, net, err, nbounds[net])
    _hold_stats(what, got, ref_stats, ref_grad, serr, pg_cond, pg_scaled)


def _stat_errs(got, ref_stats, terms):
    """(the relative error of every statistic but clipfrac, pg_loss's
    condition number, pg_loss's error on the scale of its ``terms``)."""
    # relative; a statistic that is exactly zero (pg_loss of a single
    # normalised row) must come out exactly zero
    serr = {n: abs(got[n] - float(ref_stats[n])) / abs(float(ref_stats[n]))
            if float(ref_stats[n]) != 0.0 else abs(got[n])
            for n in STAT_NAMES if n != 'clipfrac'}
    pg_ref, pg_scale = float(ref_stats['pg_loss']), float(np.mean(np.abs(terms)))
    assert abs(float(np.mean(terms)) - pg_ref) <= 1e-12 * max(pg_scale, 1e-300)    # the terms are pg_loss's
    pg_cond = pg_scale / abs(pg_ref) if pg_ref != 0.0 else 0.0
    pg_scaled = abs(got['pg_loss'] - pg_ref) / pg_scale if pg_scale > 0.0 else abs(got['pg_loss'])
    return serr, pg_cond, pg_scaled


def _hold_stats(what, got, ref_stats, ref_grad, serr, pg_cond, pg_scaled, but=()):
    """The statistics' assertions of ``_check`` (every name but those in
    ``but``, which the caller holds in another way)."""
    for name, err in serr.items():
        if name in but:
            continue
        if name != 'pg_loss' or pg_cond <= cases.PG_COND_MAX:
            assert err <= BOUND, (what, name, err)
    assert pg_scaled <= BOUND, (what, 'pg_loss on the scale of its terms', pg_scaled)
    assert got['clipfrac'] == float(np.float32(ref_stats['clipfrac'])), what
    ref_norm = float(np.sqrt(np.sum(np.asarray(ref_grad) ** 2)))
    assert abs(got['grad_norm'] - ref_norm) <= BOUND * ref_norm, what


# ------------------------------------------------------------------ 1. GAE
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
    noise = np.random.RandomState(11).normal(0, 1, (pc.ROLLOUT_K, rows, A)).astype(np.float32)
    first = eng.alloc_device_outputs()
    eng.reset_device(first)
    fields, rec, pfields, prec = eng.alloc_policy_rollout(pc.ROLLOUT_K, policy)
    eng.rollout_policy(pc.ROLLOUT_K, policy, first['obs'], torch.from_numpy(noise).cuda(),
                       fields, rec, pfields, prec)
    last = policy.forward_device(fields['obs'][pc.ROLLOUT_K - 1])
    return eng, policy, fields, pfields, last['value'], rows


@pytest.mark.parametrize('name, num_envs', [('lr_two_class_f64', 1), ('lr_two_class_f64', 3),
                                            ('lr_two_class_f64', 65), ('multi_func4', 2)])
def test_gae_parity_on_rollout_records(name, num_envs):
    import torch
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):       # the engine's launches and the learner's share it
        eng, policy, fields, pfields, last_values, rows = _rollout(name, num_envs,
                                                                   stream.cuda_stream)
        learner = PPO2Learner(policy, gamma=0.99, lam=0.95)
        rewards, dones, values = fields['reward'], fields['done'], pfields['value']
        assert tuple(rewards.shape) == (pc.ROLLOUT_K, rows)
        assert rewards.stride(0) > rows and values.stride(0) > rows      # strided records
        adv, ret = learner.gae(rewards=rewards, values=values, dones=dones, last_values=last_values)
        stream.synchronize()
    r, v, d, lv = _np(rewards), _np(values), _np(dones), _np(last_values)
    assert d.sum() == 2 * rows                      # two episode ends inside K
    ref_adv, ref_ret = gae_numpy(r, v, d, lv, 0.99, 0.95)
    for got, ref in ((_np(adv), ref_adv), (_np(ret), ref_ret)):
        err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
        print('gae', name, rows, err)
        assert err <= BOUND
    a32, r32 = gae_numpy(r, v, d, lv, 0.99, 0.95, dtype=np.float32)
    assert np.array_equal(_np(adv), a32) and np.array_equal(_np(ret), r32)
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
          max(cases.block_errs(case, _statement32(case)[0], _reference(case)[1]).values()))
    learner.close()
    learner.policy.close()


def test_gradient_parity_without_value_clip_and_normalisation():
    import torch
    case = cases.CASES[2]
    learner, inputs = _learner(case, cliprange_vf=-1.0, normalize_adv=False)
    grad, stats = learner.grad(_dev(inputs))
    torch.cuda.synchronize()
    hp = cases.HP._replace(cliprange_vf=-1.0, normalize_adv=False)
    args = [inputs[n] for n in cases.BATCH_FIELDS]
    ref = loss_grad_numpy(inputs['params'], *args, hp=hp, hidden=inputs['hidden'])
    _check(case, _np(grad), stats, ref, 'no value clip', inputs, hp)
    learner.close()
    learner.policy.close()


# ------------------------------------------------------------------- 3. idx
def test_idx_gathers_rows():
    _idx_gathers_rows(cases.CASES[3], 70)        # 130 rows as the [K R] batch


def test_idx_gathers_rows_of_shrink_then_grow_widths():
    _idx_gathers_rows(cases.SHAPE_CASES[3], 33)  # (128, 32, 64), A = 32: 33 of 40 rows


def _idx_gathers_rows(case, n_sub):
    import torch
    learner, inputs = _learner(case)
    batch = _dev(inputs)
    rs = np.random.RandomState(7)
    sub = rs.permutation(case[0])[:n_sub].astype(np.int32)
    gathered = {n: inputs[n][sub] for n in cases.BATCH_FIELDS}
    args = [gathered[n] for n in cases.BATCH_FIELDS]
    ref = loss_grad_numpy(inputs['params'], *args, hp=cases.HP, hidden=inputs['hidden'])
    g_idx, s_idx = learner.grad(batch, torch.from_numpy(sub).cuda())
    g_copy, s_copy = learner.grad(_dev(gathered))
    torch.cuda.synchronize()
    _check(case, _np(g_idx), s_idx, ref, 'idx subset', dict(inputs, **gathered))
    _check(case, _np(g_copy), s_copy, ref, 'gathered copy', dict(inputs, **gathered))
    assert np.array_equal(_np(g_idx), _np(g_copy))       # the same rows in the same order
    assert np.array_equal(_np(s_idx.tensor), _np(s_copy.tensor))
    # every row, permuted: the summation order alone differs
    perm = rs.permutation(case[0]).astype(np.int32)
    g_perm, s_perm = learner.grad(batch, torch.from_numpy(perm).cuda())
    torch.cuda.synchronize()
    _check(case, _np(g_perm), s_perm, _reference(case), 'idx permutation')
    learner.close()
    learner.policy.close()


# ---------------------------------------------------------- 4. determinism
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


# ------------------------------------------------------ 5. grid independence
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
@pytest.mark.parametrize('case, max_grad_norm, bites', [(cases.CASES[2], 0.05, True),
                                                        (cases.CASES[3], 100.0, False),
                                                        (cases.SHAPE_CASES[1], 0.05, True)],
                         ids=['clip_bites', 'clip_idle', 'clip_bites_h32x128'])
def test_three_steps_follow_the_statement(case, max_grad_norm, bites):
    import torch
    lr = 1e-2
    learner, inputs = _learner(case, max_grad_norm=max_grad_norm, lr=lr)
    batch = _dev(inputs)
    args = [inputs[n] for n in cases.BATCH_FIELDS]
    p = inputs['params'].astype(np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for t in (1, 2, 3):
        ref_stats, g = loss_grad_numpy(p, *args, hp=cases.HP, hidden=inputs['hidden'])
        assert (np.sqrt(np.sum(g * g)) > max_grad_norm) == bites
        p, m, v = adam_step_numpy(p, g, m, v, t, lr, max_grad_norm)
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
    name, E, K = 'lr_two_class_f64', 3, 10
    features, targets = pc.rollout_dataset(name)
    rows, D, A = pc.rollout_dims(name)
    params, _ = pc.rollout_policy_inputs(name)
    policy = MlpPolicy(D, A, pc.ROLLOUT_HIDDEN)
    policy.set_params(params)
    learner = PPO2Learner(policy, lr=1e-2)
    noise = torch.from_numpy(np.random.RandomState(13).normal(0, 1, (2, K, rows, A))
                             .astype(np.float32)).cuda()
    gen = torch.Generator(device='cuda')
    gen.manual_seed(5)
    env = GPUVecEnv(E, data_set=(features, targets), max_steps=4, seed=[21, 22, 23])
    env.reset()
    first = env.collect(policy, K, noise[0])
    adv, ret = learner.gae(first)
    stats = learner.update(first, noptepochs=2, nminibatches=2, generator=gen)
    second = env.collect(policy, K, noise[1])
    torch.cuda.synchronize()
    out = {'adv': _np(adv), 'ret': _np(ret), 'values0': _np(first['values']),
           'values1': _np(second['values']), 'rewards1': _np(second['rewards']),
           'params': learner.get_params(), 'stats': np.stack([_np(s.tensor) for s in stats])}
    env.close()
    learner.close()
    policy.close()
    return out


def test_collect_gae_update_collect():
    a = _closed_loop()
    assert a['stats'].shape == (4, 8) and np.isfinite(a['stats']).all()
    assert np.isfinite(a['values1']).all() and np.isfinite(a['params']).all()
    assert not np.array_equal(a['values0'], a['values1'])
    # the first value of the second rollout comes from the updated network
    assert np.max(np.abs(a['values1'][0] - a['values0'][-1])) > 0
    b = _closed_loop()
    for key in a:
        assert np.array_equal(a[key], b[key]), key


# --------------------------------------- 8. the whole update, the statement
def _strided_rollout(rollout):
    """The rollout's records on the device as ``collect`` leaves them: each
    field a [K]-row view into a wider buffer with its own pad (NaN in the
    float pads, so a read outside a record shows), ``last_values`` [R]."""
    import torch
    K = rollout['rewards'].shape[0]
    out = {}
    for extra, name in enumerate(cases.ROLLOUT_FIELDS[:-1], 3):
        a = rollout[name]
        row = a.reshape(K, -1)
        buf = np.full((K, row.shape[1] + extra), 1 if a.dtype == np.uint8 else np.nan, a.dtype)
        buf[:, :row.shape[1]] = row
        view = torch.from_numpy(buf).cuda()[:, :row.shape[1]]
        out[name] = view.unflatten(1, a.shape[1:]) if a.ndim == 3 else view
        assert out[name].stride(0) > row.shape[1]
    out['last_values'] = torch.from_numpy(rollout['last_values']).cuda()
    return out


def _update_learner(case, rollout):
    _, _, D, hidden, A, _ = case
    learner = PPO2Learner(MlpPolicy(D, A, hidden), cliprange=cases.HP.cliprange,
                          cliprange_vf=cases.HP.cliprange_vf, ent_coef=cases.HP.ent_coef,
                          vf_coef=cases.HP.vf_coef, normalize_adv=cases.HP.normalize_adv)
    learner.set_params(rollout['params'])
    return learner


def _learner_state(learner):
    import torch
    torch.cuda.synchronize()
    state = learner.get_opt_state()
    return {'params': learner.get_params(), 'm': state['m'], 'v': state['v'], 'step': state['step']}


@pytest.mark.parametrize('call', sorted(cases.UPDATE_CALLS))
@pytest.mark.parametrize('case', cases.UPDATE_CASES, ids=cases.UPDATE_CASE_IDS)
def test_update_follows_the_statement(case, call):
    """``update(perms=...)`` (GAE, flatten, two epochs of ``step`` calls over
    slices of explicit permutations, per-minibatch advantage normalisation,
    Adam's counter, the repack after every step) with a per-call ``lr`` (and,
    for ``call_clip``, ``cliprange``) against

    1. the hand-written gae -> flatten -> step(batch, perm[slice]) loop on a
       second learner: parameters, optimiser state, every step's statistics
       and ``last_returns`` bit-identical;
    2. ``ppo2_cases.update_numpy`` in float64: ``last_returns`` bit-equal to the
       float32 GAE statement and 1e-5 norm-relative to the float64 one; ``m``,
       ``v`` and ``dp = p_after - p_before`` within max(1e-5, 2 e32) in
       max|d| / max|ref|, e32 being the float32 ``update_numpy``'s own error in
       that measure; every step's statistics as ``_check`` holds them,
       clipfrac exact.

    The draw is chosen from the statements alone (``cases.update_input_holds``,
    asserted here and in test_ppo2_host.py): every minibatch row
    ``cases.MARGIN`` off the loss's kinks on the float64 trajectory, a step
    that clips, and a float32 NumPy trajectory within ``cases.F32_ROOM`` of the
    float64 one in every step's statistics and grad_norm; a seed that fails it
    failed as an input.
    lr = 1e-2 (5e-3) on purpose: at the default 2.5e-4 four steps move a
    parameter by less than a thousand float32 ulps and the float32 statement
    itself is 1e-4 off in dp.

    One exception to 1e-5 relative: the first step's approxkl.  The old policy
    is the current one there, so neglogp - old_neglogp is zero but for the
    float32 rounding of the stored actions and neglogp, and approxkl (6e-15 in
    the float64 statement, 6e-14 in the float32 one) is rounding noise with no
    digits to compare.  It is held to 0.5 (1e-5 max|neglogp|)^2, the project's
    float32 bound on the scale of what is subtracted (3e-9 here; the device
    gives 1.9e-14 at the most).

    Measured on the MI355X, worst over the six runs (smallest margin 1.7e-3,
    clipfrac up to 1.0, float32 statement's statistics and grad_norm within
    3.4e-6):

        returns  7.7e-08 norm-relative (bound 1e-5), bit-equal in float32
        dp       device 6.3e-06   e32 up to 1.7e-05   (bound max(1e-5, 2 e32))
        m        device 3.5e-06   e32 up to 4.0e-06
        v        device 5.8e-06   e32 up to 8.2e-06
        loss 2.4e-07, vf_loss 1.8e-07, entropy 5.8e-08, approxkl 2.5e-06 (steps
        after the first), grad_norm 7.0e-06, pg_loss 9.3e-06 where its condition
        number is under 50 and 2.9e-07 of mean|term| everywhere (bound 1e-5
        each); clipfrac exact
    """
    import torch
    K, R, _, hidden, _, nminibatches = case
    lr, cliprange = cases.UPDATE_CALLS[call]
    rollout, hp, lr32, ref = cases.update_reference(case, call)
    f32 = cases.update_reference(case, call, dtype=np.float32)[3]
    margin, top_clip, _ = cases.update_input_holds(rollout, hp, ref, f32)
    result = _strided_rollout(rollout)
    perms = [torch.from_numpy(p).cuda() for p in rollout['perms']]

    learner = _update_learner(case, rollout)
    stats = learner.update(result, noptepochs=cases.UPDATE_EPOCHS, nminibatches=nminibatches,
                           perms=perms, lr=lr, cliprange=cliprange)
    got = _learner_state(learner)
    got_ret = _np(learner.last_returns)
    n_steps = cases.UPDATE_EPOCHS * nminibatches
    assert len(stats) == n_steps and got['step'] == n_steps

    # 1. device against device
    loop = _update_learner(case, rollout)
    adv, ret = loop.gae(result)
    batch = loop.flatten(result, adv, ret)
    size = K * R // nminibatches
    loop_stats = [loop.step(batch, perm[b * size:(b + 1) * size], lr=lr, cliprange=cliprange)
                  for perm in perms for b in range(nminibatches)]
    want = _learner_state(loop)
    for name in ('params', 'm', 'v'):
        assert np.array_equal(got[name], want[name]), name
    assert got['step'] == want['step']
    for i, (a, b) in enumerate(zip(stats, loop_stats)):
        assert np.array_equal(_np(a.tensor), _np(b.tensor)), i
    assert np.array_equal(got_ret, _np(ret))

    # 2. device against the statement
    assert got_ret.shape == (K, R) and not np.isnan(got_ret).any()
    assert np.array_equal(got_ret, f32['returns'])
    ret_err = np.linalg.norm(got_ret - ref['returns']) / np.linalg.norm(ref['returns'])
    assert ret_err <= BOUND, ret_err
    p0 = rollout['params'].astype(np.float64)
    measures = {}
    for name in ('dp', 'm', 'v'):
        r = ref['params'] - p0 if name == 'dp' else ref[name]
        g = got['params'].astype(np.float64) - p0 if name == 'dp' else got[name]
        s = f32['params'].astype(np.float64) - p0 if name == 'dp' else f32[name]
        measures[name] = (pc.rel_err(g, r), pc.rel_err(s, r))
    print('update', case, call, 'margin %.3g, largest clipfrac %.2f, returns %.3g; '
          % (margin, top_clip, ret_err),
          ', '.join('%s device %.3g e32 %.3g' % (n, e[0], e[1]) for n, e in measures.items()))
    for name, (err, e32) in measures.items():
        assert err <= max(BOUND, 2 * e32), (name, err, e32)
    for i, (stat, ref_stats) in enumerate(zip(stats, ref['stats'])):
        what = 'update %s %s step %d' % (case, call, i)
        inputs = dict(ref['batches'][i], params=ref['before'][i], hidden=hidden)
        step_stats = stat.stats()
        serr, pg_cond, pg_scaled = _stat_errs(step_stats, ref_stats, cases.pg_terms(inputs, hp))
        norm = np.sqrt(np.sum(ref['grads'][i] ** 2))
        n32 = abs(np.sqrt(np.sum(f32['grads'][i].astype(np.float64) ** 2)) - norm) / norm
        print(what, serr, 'clipfrac %g' % step_stats['clipfrac'],
              'pg_loss: condition %.1f, |d| / mean|term| %.3g' % (pg_cond, pg_scaled),
              'grad_norm device %.3g e32 %.3g' % (abs(step_stats['grad_norm'] - norm) / norm, n32))
        _hold_stats(what, step_stats, ref_stats, ref['grads'][i], serr, pg_cond, pg_scaled,
                    but=('approxkl',) if i == 0 else ())
    top = float(np.max(np.abs(rollout['neglogps'])))
    first_kl = stats[0].stats()['approxkl']
    print('update', case, call, 'first approxkl %.3g, bound %.3g' % (first_kl, 0.5 * (BOUND * top) ** 2))
    assert first_kl <= 0.5 * (BOUND * top) ** 2, first_kl
    # the repack followed the last step
    obs = torch.from_numpy(rollout['obs'][0]).cuda()
    out = learner.policy.forward_device(obs)
    torch.cuda.synchronize()
    fwd = forward_numpy(rollout['obs'][0], None, got['params'].astype(np.float64), hidden)
    assert pc.rel_err(_np(out['action']), fwd['mean']) <= BOUND
    assert pc.rel_err(_np(out['value']), fwd['value']) <= BOUND
    for l in (learner, loop):
        l.close()
        l.policy.close()
