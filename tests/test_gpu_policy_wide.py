"""The wide policy on the device (``WideMlpPolicy``, ce_policy_create_wide,
csrc/policy_wide_kernels.h): the reference's default ``Optimize-v0`` shape,
981 -> hidden -> 490, driven closed loop.

1. Forward parity against ``forward_numpy`` in float64 on the float32-rounded
   inputs.  Bound per output array: max(1e-5, 2 e32), e32 the error of the
   NumPy float32 statement whose first-layer product is accumulated one k at a
   time in ascending order (policy_wide_cases.forward_ordered_f32) -- computed
   from NumPy alone.  1e-5 is the project's float32 bound, 2 the margin the
   learner tests give the float32 statement.
2. A wide handle at a shape the narrow kernel takes gives the narrow kernel's
   bits, for block noise, no noise and a ``DeviceRng``.
3. The generated instance is bit-equal to the explicit one fed
   ``DeviceRng.normal`` at 981 -> 490.
4. ``rollout_policy(k=10)`` on a 49 x 10 full-batch float64 engine is bit-equal
   to ten forward + step pairs, each record is ``forward_numpy`` of the
   observation it was chosen from, and the recorded env_action block replays
   to the same env records.
5. ``GPUVecEnv.collect`` and ``VecNormalize.collect`` at that shape.
6. The learners refuse a live wide handle and leave it usable.
"""
import numpy as np
import pytest

import policy_cases as pc
import policy_wide_cases as wc
import vecnorm_cases as vcases
from custom_envs_amd import _native, rng
from custom_envs_amd.policy import POLICY_FIELDS, MlpPolicy, WideMlpPolicy, forward_numpy

pytestmark = pytest.mark.gpu

SEED = (5 << 32) | 17


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _flat(params, policy):
    return np.concatenate([params[n].reshape(-1) for n in policy.params_layout()])


# ------------------------------------------------------------ 1. forward parity
@pytest.mark.parametrize('case', wc.WIDE_CASES, ids=[wc.case_id(c) for c in wc.WIDE_CASES])
def test_forward_parity(case):
    import torch
    rows, D, hidden, A = case
    obs, noise, params, ref, ref_det, bounds, e32 = wc.case_reference(case)
    policy = WideMlpPolicy(D, A, hidden, low=wc.LOW, high=wc.HIGH)
    policy.set_params(params)
    out = policy.forward_device(_dev(obs), _dev(noise))
    torch.cuda.synchronize()
    got = {k: _np(v) for k, v in out.items()}
    errs = {k: pc.rel_err(got[k], ref[k]) for k in wc.KEYS}
    print('wide forward parity', case, 'kernel', errs, 'ordered float32 statement', e32,
          'bounds', bounds)
    for key in wc.KEYS:
        assert errs[key] <= bounds[key], (key, errs[key], bounds[key])
    assert np.array_equal(got['env_action'],
                          np.clip(got['action'], np.float32(wc.LOW), np.float32(wc.HIGH)))
    clipped = float(np.mean(got['env_action'] != got['action']))
    assert 0.1 <= clipped <= 0.9, clipped

    # the deterministic policy: action == mean, neglogp the constant
    det = policy.forward_device(_dev(obs))
    torch.cuda.synchronize()
    assert pc.rel_err(_np(det['action']), ref_det['mean']) <= bounds['action']
    terms = (float(np.sum(params['logstd'].astype(np.float64))), 0.5 * A * np.log(2 * np.pi))
    assert np.all(_np(det['neglogp']) == _np(det['neglogp'])[0])
    assert abs(float(_np(det['neglogp'])[0]) - sum(terms)) <= \
        bounds['neglogp'] * (abs(terms[0]) + terms[1])
    assert np.array_equal(_np(det['value']), got['value'])

    # a device-side parameter refresh gives the same bits
    other = WideMlpPolicy(D, A, hidden, low=wc.LOW, high=wc.HIGH)
    other.set_params(_dev(_flat(params, policy)))
    again = other.forward_device(_dev(obs), _dev(noise))
    torch.cuda.synchronize()
    for key in POLICY_FIELDS:
        assert np.array_equal(_np(again[key]), got[key]), key
    policy.close()
    other.close()


# ------------------------------------------- 2. the narrow kernel's bits
@pytest.mark.parametrize('case', wc.NARROW_CASES, ids=[wc.case_id(c) for c in wc.NARROW_CASES])
def test_same_bits_as_the_narrow_kernel(case):
    import torch
    rows, D, hidden, A = case
    obs, noise, params = pc.forward_inputs(case)
    narrow = MlpPolicy(D, A, hidden, low=wc.LOW, high=wc.HIGH)
    wide = WideMlpPolicy(D, A, hidden, low=wc.LOW, high=wc.HIGH)
    g = rng.DeviceRng(SEED, 0, row_offset=3)
    g.t = 11
    dobs = _dev(obs)
    for kind, nz in (('block', _dev(noise)), ('none', None), ('generated', g)):
        outs = []
        for policy in (narrow, wide):
            policy.set_params(params)
            outs.append({k: _np(v) for k, v in policy.forward_device(dobs, nz).items()})
        torch.cuda.synchronize()
        for key in POLICY_FIELDS:
            assert np.array_equal(_bits(outs[0][key]), _bits(outs[1][key])), (kind, key)
        assert np.isfinite(outs[1]['action']).all() and np.isfinite(outs[1]['neglogp']).all()
    narrow.close()
    wide.close()


# ------------------------------------------- 3. generated == explicit
def test_generated_equals_explicit_at_the_reference_shape():
    import torch
    rows, D, hidden, A = wc.WIDE_CASES[1]
    obs, _, params = pc.forward_inputs(wc.WIDE_CASES[1])
    policy = WideMlpPolicy(D, A, hidden, low=wc.LOW, high=wc.HIGH)
    policy.set_params(params)
    g = rng.DeviceRng(SEED, 0, row_offset=77)
    g.t = 41
    block = g.normal(1, rows, A)[0]
    explicit = policy.forward_device(_dev(obs), noise=block)
    generated = policy.forward_device(_dev(obs), noise=g)
    torch.cuda.synchronize()
    assert g.t == 41
    # the 490-wide block is the statement's stream (test_gpu_rng.py's bound)
    ref = rng.normal_numpy(SEED, 41, rows, A, row_offset=77)
    assert np.abs(_np(block).astype(np.float64) - ref).max() <= 1e-5
    for name in POLICY_FIELDS:
        assert np.array_equal(_bits(_np(generated[name])), _bits(_np(explicit[name]))), name
    assert np.isfinite(_np(generated['neglogp'])).all()
    mean = policy.forward_device(_dev(obs))
    assert not np.array_equal(_np(mean['action']), _np(generated['action']))
    policy.close()


# ------------------------------------------- 4. the closed loop at 981 -> 490
def _make_engine():
    from custom_envs_amd.engine import OptimizeEngine
    features, targets = wc.dataset()
    eng = OptimizeEngine(features, targets, num_envs=wc.ENVS, batch_size=None, max_steps=4,
                         precision='f64')
    eng.seed(list(wc.SEEDS))
    assert eng.obs_dim == 981 and eng.act_dim == 490
    return eng


def _make_policy():
    params, noise = wc.rollout_inputs()
    policy = WideMlpPolicy(wc.OBS_DIM, wc.ACT_DIM, wc.HIDDEN)
    policy.set_params(params)
    return policy, params, noise


def _generator():
    g = rng.DeviceRng(SEED, 0, row_offset=5)
    g.t = 9
    return g


def _env_names(eng):
    return [n for n, _, _, _ in eng.output_fields()]


def _fused(generated):
    import torch
    eng = _make_engine()
    policy, params, noise = _make_policy()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng.set_stream(stream.cuda_stream)
        first = eng.alloc_device_outputs()
        eng.reset_device(first)
        fields, rec, pfields, prec = eng.alloc_policy_rollout(wc.ROLLOUT_K, policy)
        nz = _generator() if generated else _dev(noise)
        eng.rollout_policy(wc.ROLLOUT_K, policy, first['obs'], nz, fields, rec, pfields, prec)
        stream.synchronize()
        out = (_np(first['obs']), {n: _np(fields[n]) for n in _env_names(eng)},
               {n: _np(pfields[n]) for n in POLICY_FIELDS})
    eng.close()
    policy.close()
    return out


def _unfused(generated):
    import torch
    eng = _make_engine()
    policy, params, noise = _make_policy()
    env_rec = {n: [] for n in _env_names(eng)}
    pol_rec = {n: [] for n in POLICY_FIELDS}
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng.set_stream(stream.cuda_stream)
        out = eng.alloc_device_outputs()
        eng.reset_device(out)
        dnoise, g = _dev(noise), _generator()
        pout = policy.alloc_outputs(wc.ENVS)
        for t in range(wc.ROLLOUT_K):
            policy.forward_device(out['obs'], g if generated else dnoise[t], out=pout)
            g.t += 1
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


def _fused_cached(generated):
    if generated not in _FUSED:
        _FUSED[generated] = _fused(generated)
    return _FUSED[generated]


@pytest.mark.parametrize('generated', [False, True], ids=['block', 'generated'])
def test_fused_rollout_equals_unfused(generated):
    _, env, pol = _fused_cached(generated)
    env_ref, pol_ref = _unfused(generated)
    for n in pol_ref:
        assert np.array_equal(_bits(pol[n]), _bits(pol_ref[n])), n
    for n in env_ref:
        assert np.array_equal(env[n], env_ref[n], equal_nan=True), n
    assert env['done'].sum() == 2 * env['done'].shape[1]       # two auto-resets per env


def test_closed_loop_is_policy_then_env():
    import torch
    obs0, env, pol = _fused_cached(False)
    params, noise = wc.rollout_inputs()
    assert np.isfinite(env['obs']).all() and np.isfinite(obs0).all()
    chosen_from = np.concatenate([obs0[None], env['obs'][:-1]])
    for t in range(wc.ROLLOUT_K):
        ref = forward_numpy(chosen_from[t], noise[t], params, hidden=wc.HIDDEN)
        bounds, e32 = wc.bounds_for(chosen_from[t], noise[t], params, wc.HIDDEN, ref)
        errs = {k: pc.rel_err(pol[k][t], ref[k]) for k in wc.KEYS}
        print('wide closed loop', t, errs, 'ordered float32 statement', e32)
        for key in wc.KEYS:
            assert errs[key] <= bounds[key], (t, key, errs[key], bounds[key])
        assert np.array_equal(pol['env_action'][t], pol['action'][t])      # unbounded policy
    # the recorded env_action block, open loop, through the per-step launch form
    eng = _make_engine()
    eng.set_persistent(False)
    fields, rec = eng.alloc_rollout(wc.ROLLOUT_K)
    acts = _dev(pol['env_action'])
    torch.cuda.synchronize()          # the engine runs on its own stream
    eng.reset_device({n: v[0] for n, v in fields.items() if n != '_buffer'})
    eng.rollout_device(wc.ROLLOUT_K, acts, fields, rec)
    eng.wait()
    for n in _env_names(eng):
        assert np.array_equal(_np(fields[n]), env[n], equal_nan=True), n
    eng.close()


# ------------------------------------------------------- 5. vec-env surface
def _make_env():
    from custom_envs_amd.vectorize.gpuvecenv import GPUVecEnv
    env = GPUVecEnv(wc.ENVS, data_set=wc.dataset(), max_steps=4, seed=list(wc.SEEDS),
                    precision='f64')
    assert env.engine.obs_dim == 981 and env.engine.act_dim == 490
    return env


def test_gpuvecenv_collect():
    import torch
    K, rows, D, A = wc.ROLLOUT_K, wc.ENVS, wc.OBS_DIM, wc.ACT_DIM
    policy, params, noise = _make_policy()
    env = _make_env()
    obs0 = env.reset()
    got = env.collect(policy, K, _dev(noise))
    torch.cuda.synchronize()
    shapes = {'obs': (K, rows, D), 'actions': (K, rows, A), 'env_actions': (K, rows, A),
              'values': (K, rows), 'neglogps': (K, rows), 'rewards': (K, rows), 'dones': (K, rows),
              'last_obs': (rows, D), 'last_values': (rows,)}
    for key, shape in shapes.items():
        assert tuple(got[key].shape) == shape, key
        assert got[key].device.type == 'cuda'
    obs = _np(got['obs'])
    assert np.array_equal(obs[0], obs0)
    # obs[t + 1] is what step t returned; last_obs is record K-1's
    replay = _make_env()
    assert np.array_equal(replay.reset(), obs0)
    env_actions = _np(got['env_actions'])
    for t in range(K):
        o, r, d, _ = replay.step(env_actions[t])
        assert np.array_equal(o, obs[t + 1] if t + 1 < K else _np(got['last_obs'])), t
        assert np.array_equal(r, _np(got['rewards'])[t]) and np.array_equal(d, _np(got['dones'])[t] != 0)
    assert _np(got['dones']).sum() == 2 * rows
    assert np.array_equal(_np(got['last_values']),
                          _np(policy.forward_device(got['last_obs'].contiguous())['value']))
    # a collect after a step starts from that step's observation
    o, _, _, _ = env.step(env_actions[0])
    more = env.collect(policy, 2, _dev(noise[:2]))
    assert np.array_equal(_np(more['obs'])[0], o)
    env.close()
    replay.close()
    policy.close()


def test_vecnormalize_collect_against_the_statement():
    """The normalised rollout at 981 -> 490: the raw records are the bare
    env's under the recorded env_actions, the normalised observations and
    rewards and the moments are ``vecnormalize_numpy`` of them (tolerances of
    vecnorm_cases), and each policy record is ``forward_numpy`` of the
    normalised observation it was chosen from."""
    import torch
    from custom_envs_amd.vectorize import VecNormalize
    from custom_envs_amd.vectorize import vecnormalize as vnz
    K, rows, D, A = 6, wc.ENVS, wc.OBS_DIM, wc.ACT_DIM
    policy, params, noise = _make_policy()
    wrapped = VecNormalize(_make_env())
    first = wrapped.reset()
    res = wrapped.collect(policy, K, noise=_dev(noise[:K]))
    torch.cuda.synchronize()
    got = {n: _np(v) for n, v in res.items()}
    state = wrapped.normalizer.get_state()
    assert got['obs'].shape == (K, rows, D) and got['actions'].shape == (K, rows, A)
    assert np.array_equal(got['obs'][0], first)

    twin = _make_env()
    raw = np.asarray(twin.reset(), np.float32)
    ref_state = vnz.initial_state(rows, D)
    cur, _ = vnz.vecnormalize_numpy(ref_state, raw, reset=True)
    e_obs = e_rew = 0.0
    for t in range(K):
        assert np.array_equal(got['original_obs'][t], raw), t
        e_obs = max(e_obs, float(np.abs(got['obs'][t].astype(np.float64) - cur).max()))
        ref = forward_numpy(got['obs'][t], noise[t], params, hidden=wc.HIDDEN)
        bounds, _ = wc.bounds_for(got['obs'][t], noise[t], params, wc.HIDDEN, ref)
        for key, name in (('action', 'actions'), ('value', 'values'), ('neglogp', 'neglogps')):
            assert pc.rel_err(got[name][t], ref[key]) <= bounds[key], (t, key)
        raw, rew, done, _ = twin.step(got['env_actions'][t])
        raw = np.asarray(raw, np.float32)
        assert np.array_equal(np.asarray(rew, np.float32), got['original_rewards'][t]), t
        assert np.array_equal(done, got['dones'][t] != 0), t
        cur, rew_n = vnz.vecnormalize_numpy(ref_state, raw, rew, done)
        e_rew = max(e_rew, float(np.abs(got['rewards'][t].astype(np.float64) - rew_n).max()))
    e_obs = max(e_obs, float(np.abs(got['last_obs'].astype(np.float64) - cur).max()))
    errs = vcases.stat_errors(state, ref_state)
    print('wide vecnorm collect', errs, 'obs', e_obs, 'rew', e_rew)
    assert max(float(e) for e in errs.values()) <= vcases.STAT_TOL, errs
    assert e_obs <= vcases.OUT_TOL and e_rew <= vcases.OUT_TOL
    assert np.abs(got['obs']).max() <= 10.0 and np.abs(got['rewards']).max() <= 10.0
    assert not np.array_equal(got['obs'][1], got['original_obs'][1])
    wrapped.close()
    twin.close()
    policy.close()


# ------------------------------------------------------- 6. the learners refuse
def test_the_learners_refuse_a_live_wide_handle():
    import ctypes
    import torch
    from custom_envs_amd.a2c import A2CLearner
    from custom_envs_amd.ppo2 import PPO2Learner
    rows, D, hidden, A = wc.WIDE_CASES[1]
    obs, noise, params = pc.forward_inputs(wc.WIDE_CASES[1])
    policy = WideMlpPolicy(D, A, hidden)
    policy.set_params(params)
    before = {k: _np(v) for k, v in policy.forward_device(_dev(obs), _dev(noise)).items()}
    for cls in (PPO2Learner, A2CLearner):
        with pytest.raises(_native.NativeEngineError, match='CE_EUNSUPPORTED'):
            cls(policy)
    # the C entries themselves, with the live handle
    lib = _native.load()
    for cls in (PPO2Learner, A2CLearner):
        cfg = cls(MlpPolicy(5, 2, (32,), device=None))._cfg
        handle = ctypes.c_void_p()
        rc = getattr(lib, cls.PREFIX + '_create')(policy._h, ctypes.byref(cfg), ctypes.byref(handle))
        assert rc == _native.CE_EUNSUPPORTED and not handle.value
        msg = lib.ce_last_error()
        assert b'obs_dim <= 128' in msg and b'act_dim <= 64' in msg, msg
    after = {k: _np(v) for k, v in policy.forward_device(_dev(obs), _dev(noise)).items()}
    torch.cuda.synchronize()
    for key in POLICY_FIELDS:
        assert np.array_equal(_bits(before[key]), _bits(after[key])), key
    policy.close()
