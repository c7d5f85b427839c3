"""The device monitor behind the vec envs and ``learn``'s diagnostics: one env
with the host ``VecMonitor`` and one with ``DeviceVecMonitor``, the same seeds,
policy and noise, must write the same ``.mon.csv`` files (but column ``t``) and
answer ``env_method`` alike; ``diagnostics=True`` must report the explained
variance of each update and leave the parameters' bits alone."""
import functools

import numpy as np
import pytest

from custom_envs_amd.agents import A2C, PPO2, MlpPolicy
from custom_envs_amd.utils import utils_logging as ul

pytestmark = pytest.mark.gpu

MULTI_KEYS = ('loss', 'actions_mean', 'weights_mean', 'actions_std', 'states_mean', 'grads_mean',
              'grad_diff')
ARCH = {'net_arch': [dict(pi=[32], vf=[32])]}


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')


def _gpu_env(tmp, device, style='logging', chunk_size=1, paths=True):
    from custom_envs_amd.vectorize.gpuvecenv import GPUVecEnv
    E = 5
    mkw = {'info_keywords': ('objective', 'accuracy'), 'chunk_size': chunk_size, 'style': style,
           'device': device}
    files = [str(tmp / ('%s_%d' % ('dev' if device else 'host', i))) for i in range(E)]
    return GPUVecEnv(E, data_set='gaussians_256x10', max_steps=3, seed=list(range(70, 70 + E)),
                     monitor=(files if paths else None, mkw)), files


def _opt_env(tmp, device, style='logging', chunk_size=1):
    from custom_envs_amd.core import make
    from custom_envs_amd.vectorize.optvecenv import OptVecEnv
    from custom_envs_amd.wrappers.monitor import Monitor as SBMonitor
    E = 3
    files = [str(tmp / ('%s_opt_%d' % ('dev' if device else 'host', i))) for i in range(E)]
    target = functools.partial(make, 'MultiOptLRs-v0', problem='func4', max_batches=3)
    if style == 'sb':
        fns = [functools.partial(SBMonitor, target, f, info_keywords=MULTI_KEYS,
                                 allow_early_resets=True) for f in files]
    else:
        fns = [functools.partial(ul.Monitor, target, f, info_keywords=MULTI_KEYS,
                                 chunk_size=chunk_size) for f in files]
    env = OptVecEnv(fns, device_monitor=device)
    assert env.engine_backed
    return env, files


def _drive(env, rows, obs_dim, act_dim, low, high):
    """collect(K=7) twice, one step(), then collect_ddpg(K=4) -- 19 steps, six
    episodes of three per env -- and two more collected steps, so a seventh
    episode is left short of a chunk of three for close() to flush; returns
    the episode dicts step() reported."""
    import torch
    from custom_envs_amd import ddpg
    from custom_envs_amd.agents import init_params_numpy
    from custom_envs_amd.policy import MlpPolicy as DevicePolicy
    policy = DevicePolicy(obs_dim, act_dim, (32,), low=low, high=high)
    policy.set_params(init_params_numpy(policy.params_layout(), 3))
    gen = torch.Generator(device='cuda').manual_seed(11)
    env.reset()
    for _ in range(2):
        noise = torch.randn((7, rows, act_dim), device='cuda', generator=gen)
        env.collect(policy, 7, noise=noise)
    actions = np.random.RandomState(2).uniform(0.5, 1.0, (rows, act_dim)).astype(np.float32)
    _, _, dones, infos = env.step(actions if act_dim > 1 else actions.reshape(rows, 1))
    episodes = {i: dict(infos[i]['episode']) for i in np.flatnonzero(dones)}
    agent = ddpg.DDPGAgent(obs_dim, act_dim, (32,), scale=np.abs(low))
    agent.set_params(ddpg.init_params_numpy(obs_dim, act_dim, (32,), 4))
    memory = ddpg.ReplayMemory(8 * rows, rows, obs_dim, act_dim)
    noise = 0.1 * torch.randn((4, rows, act_dim), device='cuda', generator=gen)
    env.collect_ddpg(agent, memory, 4, noise=noise)
    env.collect(policy, 2, noise=False)
    return episodes


def _csv_rows(path):
    """The file's rows without column t, as (header, rows of strings)."""
    import pandas as pd
    frame = pd.read_csv(ul._mon_path(path), dtype=str, keep_default_na=False)
    return tuple(c for c in frame.columns if c != 't'), frame.drop(columns='t').values.tolist()


def _compare(make_env, dims, tmp_path, style, chunk_size):
    host, host_files = make_env(tmp_path, False, style, chunk_size)
    dev, dev_files = make_env(tmp_path, True, style, chunk_size)
    assert type(host.monitor) is ul.VecMonitor and type(dev.monitor) is ul.DeviceVecMonitor
    ep_host, ep_dev = _drive(host, *dims(host)), _drive(dev, *dims(dev))
    assert ep_host.keys() == ep_dev.keys() and ep_host
    for i in ep_host:
        a, b = dict(ep_host[i]), dict(ep_dev[i])
        a.pop('t'), b.pop('t')
        assert a == b
    for method in ('get_episode_rewards', 'get_episode_lengths', 'get_total_steps'):
        assert host.env_method(method) == dev.env_method(method), method
    assert [len(t) for t in host.env_method('get_episode_times')] == [
        len(t) for t in dev.env_method('get_episode_times')]
    assert sum(len(r) for r in dev.env_method('get_episode_rewards')) > len(dev_files)
    if chunk_size > 1:          # rows short of a chunk are still pending in both
        assert [len(d) for d in host.monitor.data] == [len(d) for d in dev.monitor.data]
        assert any(dev.monitor.data)
    host.close(), dev.close()   # flushes the rest
    for hf, df in zip(host_files, dev_files):
        assert _csv_rows(hf) == _csv_rows(df)
        assert len(_csv_rows(df)[1]) > 0


def _gpu_dims(env):
    eng = env.engine
    space = env.single_action_space
    return env.num_envs, eng.obs_dim, eng.act_dim, space.low.reshape(-1), space.high.reshape(-1)


def _opt_dims(env):
    eng = env._engine
    return (eng.rows, 3 * eng.max_history, 1, env.action_space.low.reshape(-1),
            env.action_space.high.reshape(-1))


@pytest.mark.parametrize('style,chunk_size', [('logging', 1), ('logging', 3), ('sb', 1), ('sb', 3)])
def test_gpuvecenv_files_equal_the_host_monitor(tmp_path, style, chunk_size):
    _compare(_gpu_env, _gpu_dims, tmp_path, style, chunk_size)


@pytest.mark.parametrize('style,chunk_size', [('logging', 1), ('logging', 3), ('sb', 1)])
def test_optvecenv_files_equal_the_host_monitor(tmp_path, style, chunk_size):
    _compare(_opt_env, _opt_dims, tmp_path, style, chunk_size)


def test_device_monitor_refuses_callbacks_and_unknown_keywords(tmp_path):
    from custom_envs_amd.vectorize.gpuvecenv import GPUVecEnv
    for mkw in ({'device': True, 'callbacks': [print]},
                {'device': True, 'info_keywords': ('loss',)}):
        with pytest.raises(ValueError):
            GPUVecEnv(2, data_set='gaussians_256x10', monitor=(None, mkw))


def test_drain_size_follows_the_finished_episodes(tmp_path):
    env, _ = _gpu_env(tmp_path, True, paths=False)
    from custom_envs_amd.agents import init_params_numpy
    from custom_envs_amd.policy import MlpPolicy as DevicePolicy
    _, D, A, low, high = _gpu_dims(env)
    policy = DevicePolicy(D, A, (32,), low=low, high=high)
    policy.set_params(init_params_numpy(policy.params_layout(), 3))
    env.reset()
    env.collect(policy, 2, noise=False)          # max_steps = 3: nobody finishes
    assert env.monitor.drained_bytes == 8
    env.collect(policy, 7, noise=False)          # steps 3, 6, 9 finish: 3 episodes per env
    rb = ul.record_dtype(2).itemsize
    assert env.monitor.drained_bytes == 16 + 3 * env.num_envs * rb
    assert env.env_method('get_episode_lengths') == [[3, 3, 3]] * env.num_envs
    env.close()


def _ev_of(result, learner, algo):
    """explained_variance_numpy of a collect result, its returns recomputed
    with the learner's NumPy statement in float64."""
    from custom_envs_amd.a2c import returns_numpy
    from custom_envs_amd.ppo2 import gae_numpy
    host = {n: result[n].cpu().numpy() for n in ('rewards', 'dones', 'values', 'last_values')}
    if algo == 'ppo2':
        _, ret = gae_numpy(host['rewards'], host['values'], host['dones'], host['last_values'],
                           gamma=learner.gamma, lam=learner.lam, dtype=np.float64)
    else:
        ret = returns_numpy(host['rewards'], host['dones'], host['last_values'],
                            gamma=learner.gamma, dtype=np.float64)
    return ul.explained_variance_numpy(host['values'], ret)


@pytest.mark.parametrize('algo', ['ppo2', 'a2c'])
@pytest.mark.parametrize('kind', ['gpu', 'opt'])
def test_learn_diagnostics(tmp_path, algo, kind, capsys):
    make_env = _gpu_env if kind == 'gpu' else _opt_env
    cls, kw = (PPO2, dict(n_steps=7, nminibatches=1, noptepochs=2)) if algo == 'ppo2' else (
        A2C, dict(n_steps=7))
    params, logs = {}, {}
    for diagnostics in (True, False):
        sub = tmp_path / str(diagnostics)
        sub.mkdir()
        env, _ = make_env(sub, True)
        model = cls(MlpPolicy, env, seed=17, policy_kwargs=ARCH, verbose=1,
                    diagnostics=diagnostics, **kw)
        seen = []

        def callback(locals_, globals_):
            result = locals_['self']._last_result
            seen.append((_ev_of(result, model.learner, algo), model.last_diagnostics))

        # keep each update's collect result where the callback finds it
        collect = env.collect

        def keeping(*a, **k):
            model._last_result = collect(*a, **k)
            return model._last_result
        env.collect = keeping
        model.learn(2 * model.n_batch, callback=callback, log_interval=1)
        params[diagnostics] = model.get_parameters()
        logs[diagnostics] = capsys.readouterr().out
        if diagnostics:
            assert len(seen) == 2
            for want_ev, diag in seen:
                assert abs(diag['explained_variance'] - want_ev) <= 1e-6, (diag, want_ev)
                assert diag['fps'] > 0 and diag['time_elapsed'] > 0
            assert seen[1][1]['total_timesteps'] == 2 * model.n_batch
            recent = list(env.monitor.recent)[-100:]
            assert recent and len(recent) == len(model.ep_info_buf)
            last = model.last_diagnostics
            assert last['ep_rewmean'] == float(np.mean([e['r'] for e in recent]))
            assert last['eplenmean'] == float(np.mean([e['l'] for e in recent]))
        else:
            assert model.last_diagnostics is None and seen[0][1] is None
        env.close()
    assert params[True].tobytes() == params[False].tobytes()
    for key in ('ep_rewmean', 'eplenmean', 'explained_variance', 'fps', 'time_elapsed',
                'total_timesteps'):
        assert key in logs[True] and key not in logs[False], key


def test_diagnostics_without_a_device_monitor(capsys):
    from custom_envs_amd.vectorize.gpuvecenv import GPUVecEnv
    env = GPUVecEnv(5, data_set='gaussians_256x10', max_steps=3, seed=list(range(5)))
    model = A2C(MlpPolicy, env, n_steps=7, seed=1, policy_kwargs=ARCH, diagnostics=True)
    assert model.last_diagnostics is None
    model.learn(model.n_batch)
    diag = model.last_diagnostics
    assert 'ep_rewmean' not in diag and 'eplenmean' not in diag
    assert np.isfinite(diag['explained_variance']) and diag['total_timesteps'] == model.n_batch
    env.close()


def test_mixed_step_and_collect_keep_one_carry(tmp_path):
    """An episode that begins in step() calls and ends inside a collect."""
    env, _ = _gpu_env(tmp_path, True, paths=False)
    from custom_envs_amd.agents import init_params_numpy
    from custom_envs_amd.policy import MlpPolicy as DevicePolicy
    E, D, A, low, high = _gpu_dims(env)
    policy = DevicePolicy(D, A, (32,), low=low, high=high)
    policy.set_params(init_params_numpy(policy.params_layout(), 3))
    env.reset()
    rewards = []
    for _ in range(2):
        _, rew, dones, _ = env.step(np.zeros((E, A), np.float32))
        rewards.append(rew.astype(np.float64))
        assert not dones.any()
    result = env.collect(policy, 2, noise=False)
    first = result['rewards'][0].cpu().numpy().astype(np.float64)
    want = (rewards[0] + rewards[1]) + first
    got = env.env_method('get_episode_rewards')
    assert [g[0] for g in got] == list(want) and env.env_method('get_episode_lengths') == [[3]] * E
    carry = env.monitor.get_state()
    assert (carry['ep_len'] == 1).all() and (carry['episode'] == 2).all()
    assert (carry['total_steps'] == 4).all()
    env.close()
