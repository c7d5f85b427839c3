"""The device-side training loop (custom_envs_amd/agents.py) and what it
stands on: ``collect`` with a ``DeviceRng``, the optimiser state in and out,
``learn`` against the hand-written collect + update loop, resume through
``save`` / ``load``, ``predict`` and the callback.  Bit-equal means equal
32-bit words."""
import numpy as np
import pytest

import policy_cases as pc
from custom_envs_amd import rng
from custom_envs_amd.agents import A2C, PPO2, MlpPolicy
from custom_envs_amd.policy import MlpPolicy as DevicePolicy

pytestmark = pytest.mark.gpu

SHAPE = 'lr_two_class_f64'
ARCH = {'net_arch': [dict(pi=[64, 64], vf=[64, 64])]}
SEED = (5 << 32) | 99


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')


def _np(t):
    return t.detach().cpu().numpy()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _env(E=8, first_seed=40):
    from custom_envs_amd.vectorize.gpuvecenv import GPUVecEnv
    features, targets = pc.rollout_dataset(SHAPE)
    return GPUVecEnv(E, data_set=(features, targets), max_steps=4,
                     seed=list(range(first_seed, first_seed + E)))


def _policy(env):
    _, D, A = pc.rollout_dims(SHAPE)
    params, _ = pc.rollout_policy_inputs(SHAPE)
    policy = DevicePolicy(D, A, pc.ROLLOUT_HIDDEN, low=-1e3, high=1e3)
    policy.set_params(params)
    return policy, params


# ------------------------------------------------ 4. collect with a DeviceRng
COLLECT_KEYS = ('obs', 'actions', 'env_actions', 'values', 'neglogps', 'rewards', 'dones',
                'last_obs', 'last_values', 'objective', 'accuracy', 'episode_len')


def test_collect_with_a_device_rng():
    import torch
    runs = []
    for _ in range(2):
        env = _env(3)
        policy, _ = _policy(env)
        g = rng.DeviceRng(SEED, 0)
        env.reset()
        first = env.collect(policy, 4, noise=g)
        assert g.t == 4
        second = env.collect(policy, 4, noise=g)
        assert g.t == 8
        torch.cuda.synchronize()
        runs.append([{k: _np(r[k]) for k in COLLECT_KEYS} for r in (first, second)])
        env.close()
        policy.close()
    for a, b in zip(*runs):
        for k in COLLECT_KEYS:
            assert _same(a[k], b[k]), k
    # the same rollouts from explicit tensors: draws 0..3, then 4..7
    env = _env(3)
    policy, _ = _policy(env)
    rows, _, A = 3, None, pc.rollout_dims(SHAPE)[2]
    g = rng.DeviceRng(SEED, 0)
    env.reset()
    for i, t in enumerate((0, 4)):
        g.t = t
        got = env.collect(policy, 4, noise=g.normal(4, rows, A))
        torch.cuda.synchronize()
        for k in COLLECT_KEYS:
            assert _same(_np(got[k]), runs[0][i][k]), (t, k)
    assert g.t == 4                       # a tensor does not advance the generator
    env.close()
    policy.close()


# ------------------------------------------------------- 5. optimiser state
def _batch_result(env, policy, k, t):
    g = rng.DeviceRng(SEED, 0)
    g.t = t
    return env.collect(policy, k, noise=g)


@pytest.mark.parametrize('algo', ['ppo2', 'a2c'])
def test_opt_state_round_trip(algo):
    import torch
    from custom_envs_amd.a2c import A2CLearner
    from custom_envs_amd.ppo2 import PPO2Learner
    env = _env(4)
    policy, params = _policy(env)
    other_policy, _ = _policy(env)
    make = (lambda p: PPO2Learner(p, lr=1e-3)) if algo == 'ppo2' else (lambda p: A2CLearner(p, lr=1e-3))
    learner = make(policy)
    env.reset()
    results = [_batch_result(env, policy, 4, 4 * i) for i in range(3)]

    def step(lrn, result, epoch):
        if algo == 'ppo2':
            perm = torch.from_numpy(rng.permutation_numpy(SEED, epoch, 16)).cuda()
            lrn.update(result, noptepochs=1, nminibatches=2, perms=[perm])
        else:
            lrn.update(result)

    step(learner, results[0], 0)
    step(learner, results[1], 1)
    state = learner.get_opt_state()
    assert set(state) == set(learner.OPT_BLOCKS) | {'step'}
    assert state['step'] == (4 if algo == 'ppo2' else 0)
    for name in learner.OPT_BLOCKS:
        assert state[name].dtype == np.float32 and state[name].shape == (learner.n_params,)
        assert np.isfinite(state[name]).all() and np.abs(state[name]).max() > 0
    fresh = make(other_policy)
    fresh.set_params(learner.get_params())
    fresh.set_opt_state(state)
    step(learner, results[2], 2)
    step(fresh, results[2], 2)
    torch.cuda.synchronize()
    assert _same(learner.get_params(), fresh.get_params())
    a, b = learner.get_opt_state(), fresh.get_opt_state()
    assert a['step'] == b['step']
    for name in learner.OPT_BLOCKS:
        assert _same(a[name], b[name]), name
    # without the state the next step differs (the test can fail)
    bare = make(_policy(env)[0])
    bare.set_params(fresh.get_params())
    step(bare, results[2], 2)
    step(fresh, results[2], 2)
    torch.cuda.synchronize()
    assert not _same(bare.get_params(), fresh.get_params())
    with pytest.raises(ValueError, match='shape'):
        fresh.set_opt_state(dict(state, **{learner.OPT_BLOCKS[0]: state[learner.OPT_BLOCKS[0]][:-1]}))
    env.close()


# ------------------------------------------- 6. learn == the hand-written loop
def _hand_ppo2(seed, n_updates, E=8, n_steps=4, nminibatches=2, noptepochs=2, lr=2.5e-4):
    """collect(noise = normal_numpy uploaded), update(perms = permutation_numpy
    uploaded) on an equally seeded env, from the same initial parameters."""
    import torch
    from custom_envs_amd.agents import init_params_numpy
    from custom_envs_amd.ppo2 import PPO2Learner
    env = _env(E)
    _, D, A = pc.rollout_dims(SHAPE)
    policy = DevicePolicy(D, A, (64, 64), low=-1e3, high=1e3)
    learner = PPO2Learner(policy, lr=lr)
    learner.set_params(init_params_numpy(policy.params_layout(), seed))
    env.reset()
    t = epoch = 0
    for _ in range(n_updates):
        noise = np.stack([rng.normal_numpy(seed, t + s, E, A, dtype=np.float32)
                          for s in range(n_steps)])
        # the statement is float64; the device's float32 values are what the
        # kernel uses, so the uploaded tensor must hold those bits
        g = rng.DeviceRng(seed, 0)
        g.t = t
        dev_noise = g.normal(n_steps, E, A)
        assert np.abs(_np(dev_noise) - noise).max() <= 1e-5
        result = env.collect(policy, n_steps, noise=dev_noise)
        t += n_steps
        perms = []
        for _ in range(noptepochs):
            perms.append(torch.from_numpy(rng.permutation_numpy(seed, epoch, E * n_steps)).cuda())
            epoch += 1
        learner.update(result, noptepochs=noptepochs, nminibatches=nminibatches, perms=perms)
    torch.cuda.synchronize()
    out = learner.get_params()
    env.close()
    return out


def _learn_ppo2(seed, n_updates, **kw):
    env = _env(8)
    model = PPO2(MlpPolicy, env, n_steps=4, nminibatches=2, noptepochs=2, seed=seed,
                 policy_kwargs=ARCH, **kw)
    assert model.n_batch == 32
    assert model.learn(n_updates * 32) is model
    assert model.num_timesteps == n_updates * 32
    assert model.rng.t == 4 * n_updates and model.rng.epoch == 2 * n_updates
    out = model.get_parameters()
    env.close()
    return out


def test_ppo2_learn_equals_hand_written_loop():
    got = _learn_ppo2(SEED, 2)
    assert np.isfinite(got).all()
    assert _same(got, _hand_ppo2(SEED, 2))
    assert _same(got, _learn_ppo2(SEED, 2))              # the same seed twice
    assert not _same(got, _learn_ppo2(SEED + 1, 2))      # another seed
    from custom_envs_amd.agents import init_params_numpy
    assert not _same(got, init_params_numpy(DevicePolicy(41, 20, (64, 64), device=None).params_layout(),
                                            SEED))       # it learnt something


@pytest.mark.parametrize('schedule', ['constant', 'linear'])
def test_a2c_learn_equals_hand_written_loop(schedule):
    import torch
    from custom_envs_amd.a2c import A2CLearner
    from custom_envs_amd.agents import init_params_numpy
    E, n_steps, n_updates, lr = 8, 5, 3, 7e-4

    def learn(seed):
        env = _env(E)
        model = A2C(MlpPolicy, env, n_steps=n_steps, lr_schedule=schedule, learning_rate=lr,
                    seed=seed, policy_kwargs=ARCH)
        model.learn(n_updates * E * n_steps)
        out = model.get_parameters()
        env.close()
        return out

    got = learn(SEED)
    env = _env(E)
    _, D, A = pc.rollout_dims(SHAPE)
    policy = DevicePolicy(D, A, (64, 64), low=-1e3, high=1e3)
    learner = A2CLearner(policy, lr=lr)
    learner.set_params(init_params_numpy(policy.params_layout(), SEED))
    env.reset()
    total = n_updates * E * n_steps
    for u in range(1, n_updates + 1):
        g = rng.DeviceRng(SEED, 0)
        g.t = (u - 1) * n_steps
        result = env.collect(policy, n_steps, noise=g.normal(n_steps, E, A))
        rate = lr if schedule == 'constant' else lr * (1.0 - (u * E * n_steps - 1) / total)
        learner.update(result, lr=rate)
    torch.cuda.synchronize()
    assert np.isfinite(got).all()
    assert _same(got, learner.get_params())
    assert _same(got, learn(SEED))
    assert not _same(got, learn(SEED + 1))
    env.close()


def test_a2c_schedules_differ():
    def learn(schedule):
        env = _env(8)
        model = A2C(MlpPolicy, env, lr_schedule=schedule, seed=SEED, policy_kwargs=ARCH)
        model.learn(3 * 40)
        out = model.get_parameters()
        env.close()
        return out
    assert not _same(learn('constant'), learn('linear'))


# ----------------------------------------------------------------- 7. resume
@pytest.mark.parametrize('cls,kw', [(PPO2, dict(n_steps=4, nminibatches=2, noptepochs=2)),
                                    (A2C, dict(n_steps=5))])
def test_resume_through_save_and_load(cls, kw, tmp_path):
    env = _env(8)
    whole = cls(MlpPolicy, env, seed=SEED, policy_kwargs=ARCH, **kw)
    nb = whole.n_batch
    whole.learn(4 * nb)
    want, want_opt = whole.get_parameters(), whole.get_opt_state()
    env.close()

    env = _env(8)
    first = cls(MlpPolicy, env, seed=SEED, policy_kwargs=ARCH, **kw)
    first.learn(2 * nb)
    path = str(tmp_path / 'half')
    first.save(path)
    second = cls.load(path, env=env)
    assert second.num_timesteps == 2 * nb and second.rng.state() == first.rng.state()
    second.learn(2 * nb, reset_num_timesteps=False)
    assert second.num_timesteps == 4 * nb
    assert _same(second.get_parameters(), want)
    got_opt = second.get_opt_state()
    assert got_opt['step'] == want_opt['step']
    for name in second.learner.OPT_BLOCKS:
        assert _same(got_opt[name], want_opt[name]), name
    env.close()


# ---------------------------------------------------------------- 8. predict
def test_predict():
    import torch
    env = _env(8)
    model = PPO2(MlpPolicy, env, n_steps=4, nminibatches=2, seed=SEED, policy_kwargs=ARCH)
    obs = np.array(env.reset())
    model.learn(32)
    t, epoch = model.rng.t, model.rng.epoch
    actions, state = model.predict(obs, deterministic=True)
    assert state is None and isinstance(actions, np.ndarray) and actions.shape == (8, 20)
    ref = model.policy.forward_numpy(obs, None, params=model.get_parameters())
    clipped = np.clip(ref['mean'], -1e3, 1e3)
    assert np.abs(actions - clipped).max() <= 1e-5 * np.abs(clipped).max()
    one, _ = model.predict(obs[3], deterministic=True)
    assert one.shape == (20,) and _same(one, actions[3])
    on_device, _ = model.predict(torch.from_numpy(obs).cuda(), deterministic=True)
    assert torch.is_tensor(on_device) and _same(_np(on_device), actions)
    # stochastic: its own stream and counter; training's position is untouched
    s1, _ = model.predict(obs)
    s2, _ = model.predict(obs)
    assert (model.rng.t, model.rng.epoch) == (t, epoch) and model.rng.predict_t == 2
    assert not _same(s1, s2) and not _same(s1, actions)
    noise = rng.normal_numpy(SEED, 0, 8, 20, purpose=rng.PREDICT)
    std = np.exp(model.get_parameters()[-20:].astype(np.float64))
    assert np.abs(s1 - np.clip(ref['mean'] + std * noise, -1e3, 1e3)).max() <= 1e-4
    # a model loaded without an env predicts the same and refuses to learn
    import io
    buf = io.BytesIO()
    model.save(buf)
    alone = PPO2.load(io.BytesIO(buf.getvalue()))
    assert _same(alone.predict(obs, deterministic=True)[0], actions)
    with pytest.raises(RuntimeError, match='needs an env'):
        alone.learn(32)
    env.close()


def test_predict_clips_to_the_action_space():
    import functools
    from custom_envs_amd.envs.multioptlrs import MultiOptLRs
    from custom_envs_amd.vectorize.optvecenv import OptVecEnv
    env = OptVecEnv([functools.partial(MultiOptLRs, max_batches=4) for _ in range(2)])
    assert env.engine_backed
    model = A2C(MlpPolicy, env, seed=SEED, policy_kwargs=ARCH)
    assert model.spec.rows == env.num_envs and model.spec.act_dim == 1
    flat = model.get_parameters()
    off, shape = model.policy.params_layout()['pi/b_out']
    flat[off] = -5e3                                  # below the space's low of -1e3
    model.set_parameters(flat)
    obs = np.array(env.reset())
    actions, _ = model.predict(obs, deterministic=True)
    assert actions.shape == (env.num_envs, 1) and np.all(actions == np.float32(-1e3))
    model.learn(2 * model.n_batch)                    # the multi engine's loop runs too
    assert model.num_timesteps == 2 * model.n_batch
    env.close()


# ----------------------------------------------------------- 9. the callback
def test_callback_stops_and_exceptions_propagate():
    env = _env(8)
    model = PPO2(MlpPolicy, env, n_steps=4, nminibatches=2, noptepochs=1, seed=SEED,
                 policy_kwargs=ARCH)
    seen = []

    def stop_at_two(locals_, globals_):
        assert locals_['self'] is model
        seen.append((locals_['update'], locals_['self'].num_timesteps))
        return False if locals_['update'] == 2 else None

    model.learn(5 * 32, callback=stop_at_two)
    assert seen == [(1, 32), (2, 64)] and model.num_timesteps == 64

    class Pruned(Exception):
        pass

    def prune(locals_, globals_):
        raise Pruned('trial pruned at update %d' % locals_['update'])

    with pytest.raises(Pruned):
        model.learn(3 * 32, callback=prune, reset_num_timesteps=False)
    assert model.num_timesteps == 96
    # the env still steps, from the observation the loop left
    obs, rewards, dones, infos = env.step(np.zeros((8, 20), np.float32))
    assert obs.shape == (8, 41) and np.isfinite(obs).all() and len(infos) == 8
    model.learn(32, callback=lambda l, g: True)      # and the model still learns
    assert model.num_timesteps == 32
    env.close()
