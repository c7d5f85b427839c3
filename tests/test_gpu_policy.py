"""The device-side MLP policy (ce_policy_*, csrc/policy_kernels.h) and the
closed-loop K-step rollout (ce_rollout_policy / ce_multi_rollout_policy).

1. Forward parity: the fused kernel against ``forward_numpy`` in float64 on
   the float32-rounded inputs, max|d| / max|ref| <= 1e-5 over each whole
   output array (the project's float32 bound; a float32 NumPy evaluation of
   the same inputs sits at <= 4.1e-6 from the float64 one), at row counts
   below, at and past the 32-row tile, 1- to 64-wide heads, 1 to 3 hidden
   layers and the widest supported network, and at unequal and 96-wide layers
   (policy_cases.FORWARD_SHAPE_CASES); the clip bit-exact; noise=None.
2. Fused equals unfused, bit for bit: ``rollout_policy(k=10)`` against ten
   ``forward_device`` + ``step_device`` pairs on an identically seeded engine.
3. The closed loop is policy o env: every recorded action / value / neglogp
   is ``forward_numpy`` of the recorded observation it was chosen from, and
   the recorded env_action block replayed open loop through ``rollout_device``
   gives the same env records bit for bit.
4. The vec-env surface: ``GPUVecEnv.collect`` / ``OptVecEnv.collect``.
"""
import csv

import numpy as np
import pytest

import policy_cases as pc
from custom_envs_amd.policy import POLICY_FIELDS, MlpPolicy, forward_numpy

pytestmark = pytest.mark.gpu

BOUND = 1e-5


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------ 1. forward parity
@pytest.mark.parametrize('case', pc.FORWARD_CASES + pc.FORWARD_SHAPE_CASES,
                         ids=pc.FORWARD_IDS + pc.FORWARD_SHAPE_IDS)
def test_forward_parity(case):
    import torch
    rows, D, hidden, A = case
    obs, noise, params = pc.forward_inputs(case)
    policy = MlpPolicy(D, A, hidden, low=-0.5, high=0.5)
    policy.set_params(params)
    ref = policy.forward_numpy(obs, noise, dtype=np.float64)
    out = policy.forward_device(torch.from_numpy(obs).cuda(), torch.from_numpy(noise).cuda())
    torch.cuda.synchronize()
    got = {k: _np(v) for k, v in out.items()}
    errs = {k: pc.rel_err(got[k], ref[k]) for k in ('action', 'value', 'neglogp')}
    print('forward parity', case, errs)
    for key, err in errs.items():
        assert err <= BOUND, (key, err)
    assert np.array_equal(got['env_action'], np.clip(got['action'], np.float32(-0.5), np.float32(0.5)))
    clipped = float(np.mean(got['env_action'] != got['action']))
    assert 0.1 <= clipped <= 0.9, clipped

    # the deterministic policy: action == mean, neglogp the constant
    det = policy.forward_device(torch.from_numpy(obs).cuda())
    torch.cuda.synchronize()
    ref_det = policy.forward_numpy(obs, None, dtype=np.float64)
    assert pc.rel_err(_np(det['action']), ref_det['mean']) <= BOUND
    terms = (float(np.sum(params['logstd'].astype(np.float64))), 0.5 * A * np.log(2 * np.pi))
    assert np.all(_np(det['neglogp']) == _np(det['neglogp'])[0])
    # relative to the terms' size (their sum can cancel)
    assert abs(float(_np(det['neglogp'])[0]) - sum(terms)) <= BOUND * (abs(terms[0]) + terms[1])
    assert np.array_equal(_np(det['value']), got['value'])

    # a device-side parameter refresh gives the same bits
    flat = torch.from_numpy(np.concatenate([params[n].reshape(-1) for n in policy.params_layout()])).cuda()
    other = MlpPolicy(D, A, hidden, low=-0.5, high=0.5)
    other.set_params(flat)
    again = other.forward_device(torch.from_numpy(obs).cuda(), torch.from_numpy(noise).cuda())
    torch.cuda.synchronize()
    for key in POLICY_FIELDS:
        assert np.array_equal(_np(again[key]), got[key]), key
    policy.close()
    other.close()


# ------------------------------------------------------- rollouts: shared runs
def _make_engine(name):
    kind, kw = pc.ROLLOUT_SHAPES[name]
    if kind == 'optimize':
        from custom_envs_amd.engine import OptimizeEngine
        features, targets = pc.rollout_dataset(name)
        eng = OptimizeEngine(features, targets, num_envs=len(kw['seeds']),
                             batch_size=kw['batch_size'], max_steps=4)
        eng.seed(list(kw['seeds']))
        return eng
    from custom_envs_amd.multi_engine import MultiOptEngine
    return MultiOptEngine(kw['num_envs'], kw['problem'], max_batches=4, max_history=5)


def _env_names(eng):
    return [n for n, _, _, _ in eng.output_fields()]


def _make_policy(name):
    rows, D, A = pc.rollout_dims(name)
    params, noise = pc.rollout_policy_inputs(name)
    policy = MlpPolicy(D, A, pc.ROLLOUT_HIDDEN)
    policy.set_params(params)
    return policy, params, noise


def _fused(name):
    """rollout_policy(k=10): (obs0, env records, policy records) as numpy."""
    import torch
    eng = _make_engine(name)
    policy, params, noise = _make_policy(name)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng.set_stream(stream.cuda_stream)
        first = eng.alloc_device_outputs()
        eng.reset_device(first)
        fields, rec, pfields, prec = eng.alloc_policy_rollout(pc.ROLLOUT_K, policy)
        eng.rollout_policy(pc.ROLLOUT_K, policy, first['obs'], torch.from_numpy(noise).cuda(),
                           fields, rec, pfields, prec)
        stream.synchronize()
        out = (_np(first['obs']), {n: _np(fields[n]) for n in _env_names(eng)},
               {n: _np(pfields[n]) for n in POLICY_FIELDS})
    eng.close()
    policy.close()
    return out


def _unfused(name):
    """Ten forward_device + step_device pairs from Python."""
    import torch
    eng = _make_engine(name)
    policy, params, noise = _make_policy(name)
    rows = pc.rollout_dims(name)[0]
    env_rec = {n: [] for n in _env_names(eng)}
    pol_rec = {n: [] for n in POLICY_FIELDS}
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng.set_stream(stream.cuda_stream)
        out = eng.alloc_device_outputs()
        eng.reset_device(out)
        dnoise = torch.from_numpy(noise).cuda()
        pout = policy.alloc_outputs(rows)
        for t in range(pc.ROLLOUT_K):
            policy.forward_device(out['obs'], dnoise[t], out=pout)
            eng.step_device(pout['env_action'], out)
            stream.synchronize()
            for n in env_rec:
                env_rec[n].append(_np(out[n]).copy())
            for n in pol_rec:
                pol_rec[n].append(_np(pout[n]).copy())
    eng.close()
    policy.close()
    return {n: np.stack(v) for n, v in env_rec.items()}, {n: np.stack(v) for n, v in pol_rec.items()}


_FUSED = {}


def _fused_cached(name):
    if name not in _FUSED:
        _FUSED[name] = _fused(name)
    return _FUSED[name]


# ------------------------------------------- 2. fused == unfused, bit for bit
@pytest.mark.parametrize('name', sorted(pc.ROLLOUT_SHAPES))
def test_fused_rollout_equals_unfused(name):
    _, env, pol = _fused_cached(name)
    env_ref, pol_ref = _unfused(name)
    for n in pol_ref:
        assert np.array_equal(pol[n], pol_ref[n]), n
    for n in env_ref:
        assert np.array_equal(env[n], env_ref[n], equal_nan=True), n
    assert env['done'].sum() == 2 * env['done'].shape[1]       # two auto-resets per env


# ------------------------------------------- 3. the closed loop is policy o env
@pytest.mark.parametrize('name', sorted(pc.ROLLOUT_SHAPES))
def test_closed_loop_is_policy_then_env(name):
    import torch
    obs0, env, pol = _fused_cached(name)
    params, noise = pc.rollout_policy_inputs(name)
    assert np.isfinite(env['obs']).all() and np.isfinite(obs0).all()
    chosen_from = np.concatenate([obs0[None], env['obs'][:-1]])
    for t in range(pc.ROLLOUT_K):
        ref = forward_numpy(chosen_from[t], noise[t], params, hidden=pc.ROLLOUT_HIDDEN)
        errs = {k: pc.rel_err(pol[k][t], ref[k]) for k in ('action', 'value', 'neglogp')}
        print('closed loop', name, t, errs)
        for key, err in errs.items():
            assert err <= BOUND, (t, key, err)
        assert np.array_equal(pol['env_action'][t], pol['action'][t])      # unbounded policy
    # the recorded env_action block, open loop, through the existing rollout.
    # The per-step launch form: rollout_policy steps with the per-step kernel,
    # and the persistent K-step kernel is bit-equal to it only at the shapes
    # where both run the same row-tile form (tests/test_gpu_persist.py).
    eng = _make_engine(name)
    eng.set_persistent(False)
    fields, rec = eng.alloc_rollout(pc.ROLLOUT_K)
    acts = torch.from_numpy(np.ascontiguousarray(pol['env_action'])).cuda()
    torch.cuda.synchronize()          # the engine runs on its own stream
    eng.reset_device({n: v[0] for n, v in fields.items() if n != '_buffer'})
    eng.rollout_device(pc.ROLLOUT_K, acts, fields, rec)
    eng.wait()
    for n in _env_names(eng):
        assert np.array_equal(_np(fields[n]), env[n], equal_nan=True), n
    eng.close()


# ------------------------------------------------------- 4. vec-env surface
def _mon_rows(path):
    """The .mon.csv rows without the wall-clock column t."""
    with open(path) as f:
        lines = [line for line in f if not line.startswith('#')]
    rows = list(csv.DictReader(lines))
    assert rows, path
    return [{k: v for k, v in row.items() if k != 't'} for row in rows]


def _check_collect(make_env, policy, rows, D, A, K, tmp_path, info_names):
    import torch
    noise = torch.from_numpy(np.random.RandomState(9).normal(0, 1, (K, rows, A)).astype(np.float32)).cuda()
    env = make_env(str(tmp_path / 'a'))
    obs0 = env.reset()
    got = env.collect(policy, K, noise)
    torch.cuda.synchronize()
    shapes = {'obs': (K, rows, D), 'actions': (K, rows, A), 'env_actions': (K, rows, A),
              'values': (K, rows), 'neglogps': (K, rows), 'rewards': (K, rows), 'dones': (K, rows),
              'last_obs': (rows, D), 'last_values': (rows,)}
    for key, shape in shapes.items():
        assert tuple(got[key].shape) == shape, key
        assert got[key].device.type == 'cuda'
    for key in info_names:
        assert got[key].shape[0] == K, key
    obs = _np(got['obs'])
    assert np.array_equal(obs[0], obs0)
    # obs[t + 1] is what step t returned; last_obs is record K-1's
    replay = make_env(str(tmp_path / 'b'))
    assert np.array_equal(replay.reset(), obs0)
    env_actions = _np(got['env_actions'])
    for t in range(K):
        o, r, d, _ = replay.step(env_actions[t])
        assert np.array_equal(o, obs[t + 1] if t + 1 < K else _np(got['last_obs'])), t
        assert np.array_equal(r, _np(got['rewards'])[t]) and np.array_equal(d, _np(got['dones'])[t] != 0)
    # a collect after a step starts from that step's observation
    o, _, _, _ = env.step(env_actions[0])
    more = env.collect(policy, 2, noise[:2])
    assert np.array_equal(_np(more['obs'])[0], o)
    o2, _, _, _ = replay.step(env_actions[0])
    assert np.array_equal(o2, o)
    for t in range(2):                       # both envs have now taken K + 3 steps
        o2, _, _, _ = replay.step(_np(more['env_actions'])[t])
    assert np.array_equal(o2, _np(more['last_obs']))
    env.close()
    replay.close()
    return got


def test_gpuvecenv_collect(tmp_path):
    from custom_envs_amd.vectorize.gpuvecenv import GPUVecEnv
    E, K = 3, 6
    features, targets = pc.rollout_dataset('lr_two_class_f64')
    rows, D, A = pc.rollout_dims('lr_two_class_f64')
    policy, params, _ = _make_policy('lr_two_class_f64')

    def make_env(prefix):
        paths = ['%s_%d' % (prefix, i) for i in range(E)]
        return GPUVecEnv(E, data_set=(features, targets), max_steps=4, seed=[21, 22, 23],
                         monitor=(paths, dict(info_keywords=('objective', 'accuracy'))))

    got = _check_collect(make_env, policy, rows, D, A, K, tmp_path,
                         ('objective', 'accuracy', 'episode_len'))
    assert np.array_equal(_np(got['last_values']),
                          _np(policy.forward_device(got['last_obs'].contiguous())['value']))
    for i in range(E):
        a, b = _mon_rows('%s_%d.mon.csv' % (tmp_path / 'a', i)), _mon_rows('%s_%d.mon.csv' % (tmp_path / 'b', i))
        assert len(a) >= 1 and a == b, i
    policy.close()


def test_optvecenv_collect(tmp_path):
    import functools
    from custom_envs_amd.envs.multioptlrs import MultiOptLRs
    from custom_envs_amd.utils.utils_logging import Monitor
    from custom_envs_amd.vectorize.optvecenv import OptVecEnv
    E, K = 3, 6
    policy, params, _ = _make_policy('multi_func')
    rows, D, A = pc.rollout_dims('multi_func')

    def make_env(prefix):
        fns = [functools.partial(Monitor, functools.partial(MultiOptLRs, max_batches=4),
                                 '%s_%d' % (prefix, i)) for i in range(E)]
        env = OptVecEnv(fns)
        assert env.engine_backed and env.monitor is not None
        return env

    _check_collect(make_env, policy, rows, D, A, K, tmp_path, ('info', 'episode_len'))
    for i in range(E):
        a, b = _mon_rows('%s_%d.mon.csv' % (tmp_path / 'a', i)), _mon_rows('%s_%d.mon.csv' % (tmp_path / 'b', i))
        assert len(a) >= 1 and a == b, i
    policy.close()


def test_rollout_policy_refusals(lr_dataset):
    """CE_ESTATE before the first reset; compact outputs and a mismatched
    policy are refused before any launch."""
    import torch
    from custom_envs_amd import _native
    from custom_envs_amd.engine import OptimizeEngine
    eng = OptimizeEngine(*lr_dataset, num_envs=4)
    policy = MlpPolicy(eng.obs_dim, eng.act_dim, (32,))
    fields, rec, pfields, prec = eng.alloc_policy_rollout(2, policy)
    obs0 = torch.zeros((4, eng.obs_dim), dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()          # the engine runs on its own stream
    with pytest.raises(_native.NativeEngineError, match='CE_ESTATE'):
        eng.rollout_policy(2, policy, obs0, None, fields, rec, pfields, prec)
    eng.reset_device({n: v[0] for n, v in fields.items() if n != '_buffer'})
    eng.wait()
    obs0.copy_(fields['obs'][0])
    torch.cuda.synchronize()
    small = MlpPolicy(eng.obs_dim - 1, eng.act_dim, (32,))
    with pytest.raises(ValueError, match='the policy maps'):
        eng.rollout_policy(2, small, obs0, None, fields, rec, pfields, prec)
    eng.rollout_policy(2, policy, obs0, None, fields, rec, pfields, prec)     # deterministic
    eng.wait()
    assert np.array_equal(_np(pfields['action']), _np(pfields['env_action']))
    eng.set_compact_outputs(True)
    with pytest.raises(ValueError, match='compact'):
        eng.rollout_policy(2, policy, obs0, None, fields, rec, pfields, prec)
    for p in (policy, small):
        p.close()
    eng.close()
