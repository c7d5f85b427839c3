"""``OptVecEnv``: multi-agent envs flattened to one VecEnv row per agent.

Reference: custom_envs/vectorize/optvecenv.py:10-91.  ``OptVecEnv(
environment_fns, callbacks=())`` keeps its constructor, ``agent_no_list``,
``num_envs = sum of agents``, per-agent spaces, rows in sorted agent-name
order, reward/done/info replicated per agent, and ``callbacks(states,
rewards, terminals, infos)`` after each step.

Engine path: when every factory builds the same MultiOptLRs-v0 spec --
``partial(make, 'MultiOptLRs-v0', **kw)``, ``partial(MultiOptLRs, **kw)``,
or the scripts' ``partial(Monitor, make(...), log_path, ...)`` (run_multiagent_
exp_single.py:78-86) -- all envs run in ONE fused kernel per step and the
Monitors become one ``VecMonitor``.  Anything else runs the reference's
host path: one worker thread per env around an ``OptEnvRunner``.
"""
import functools

import numpy as np

from custom_envs_amd.spaces import Box
from custom_envs_amd.vectorize.concurrent import ThreadVecEnv


def flatten_dictionary(dictionary):
    """Values of a per-agent dict in sorted-name order (optvecenv.py:10-14)."""
    return [dictionary[name] for name in sorted(dictionary)]


class OptEnvRunner:
    """One multi-agent env seen as rows (optvecenv.py:17-54)."""

    def __init__(self, environment_fn):
        env = environment_fn()
        self._environment = env
        self._names = sorted(env.action_space.spaces)
        first = self._names[0]
        self.observation_space = env.observation_space.spaces[first]
        self.action_space = env.action_space.spaces[first]
        self._num_agents = len(env.observation_space.spaces)

    def reset(self):
        return flatten_dictionary(self._environment.reset())

    def step(self, actions):
        states, reward, terminal, info = self._environment.step(
            dict(zip(self._names, actions)))
        n = self._num_agents
        return flatten_dictionary(states), [reward] * n, [terminal] * n, [info] * n

    def close(self):
        self._environment.close()

    def __getattr__(self, attr):
        if attr.startswith('_'):
            raise AttributeError(attr)
        return getattr(self._environment, attr)


def _env_spec(obj):
    """MultiOptLRs kwargs an object or factory stands for, else None:
    an instance, ``partial(MultiOptLRs, **kw)`` or ``partial(make | gym.make,
    'MultiOptLRs-v0', **kw)`` (search_optimize_hyperparam.py:100-103)."""
    from custom_envs_amd.core import make_request
    from custom_envs_amd.envs.multioptlrs import MultiOptLRs
    if isinstance(obj, MultiOptLRs):
        return dict(obj.spec_kwargs), obj
    if isinstance(obj, functools.partial) and obj.func is MultiOptLRs and not obj.args:
        return dict(obj.keywords), None
    req = make_request(obj)
    if req is not None and req[0] == 'MultiOptLRs-v0':
        return req[1], None
    return None


def _batch_request(environment_fns):
    """(env kwargs, monitor settings or None, built envs to close) or None."""
    from custom_envs_amd.vectorize.concurrent import monitor_parts, monitor_request, spec_key
    keys, specs, monitors, built = [], [], [], []
    for fn in environment_fns:
        target, monitor = monitor_parts(fn)
        spec = _env_spec(target)
        if spec is None:
            return None
        kwargs, instance = spec
        keys.append(spec_key(kwargs))
        specs.append(kwargs)
        monitors.append(monitor)
        if instance is not None:
            built.append(instance)
    if not specs or len(set(keys)) != 1:
        return None
    mon = monitor_request(monitors)
    if mon is False:
        return None
    return specs[0], mon, built


class _RowInfos:
    """Per-row info dicts, one dict object per env shared by its agent rows."""

    def __init__(self, info, rewards, dones, lengths, n_agents, episodes):
        self._info, self._rewards, self._dones = info, rewards, dones
        self._lengths, self._n = lengths, n_agents
        self._episodes = episodes
        self._cache = {}

    def env_info(self, env):
        if env not in self._cache:
            from custom_envs_amd.envs.multioptlrs import info_dict
            d = info_dict(self._info[env], bool(self._dones[env]), float(self._rewards[env]),
                          int(self._lengths[env]))
            if env in self._episodes:
                d['episode'] = self._episodes[env]
            self._cache[env] = d
        return self._cache[env]

    def per_env(self):
        """Indexable view: env index -> that env's info dict."""
        rows = self

        class _View:
            def __getitem__(self, env):
                return rows.env_info(env)

            def __len__(self):
                return len(rows._info)
        return _View()

    def __len__(self):
        return len(self._info) * self._n

    def __getitem__(self, row):
        if isinstance(row, slice):
            return [self[r] for r in range(*row.indices(len(self)))]
        if row < 0:
            row += len(self)
        return self.env_info(row // self._n)

    def __iter__(self):
        return (self[r] for r in range(len(self)))


class OptVecEnv:
    def __init__(self, environment_fns, callbacks=(), device_monitor=False):
        """``device_monitor``: on the engine path, the ``partial(Monitor, ...)``
        factories become one ``utils_logging.DeviceVecMonitor`` instead of one
        ``VecMonitor``: the episode bookkeeping of ``collect`` / ``collect_ddpg``
        runs on the device (Monitor ``callbacks`` raise ``ValueError``)."""
        self.callbacks = callbacks
        self.closed = False
        self.waiting = False
        request = _batch_request(environment_fns)
        self._engine = self._host = self.monitor = None
        self._last_obs = None      # what collect() starts from (engine path)
        if request is not None:
            from custom_envs_amd.multi_engine import create_engine
            from custom_envs_amd.utils.utils_logging import make_vec_monitor
            kwargs, mon, built = request
            for env in built:      # single-env engines the caller built eagerly
                env.close()
            E = len(environment_fns)
            self._engine = create_engine(E, **kwargs)
            P, H = self._engine.n_params, self._engine.max_history
            self.agent_no_list = [P] * E
            self.observation_space = Box(low=-1e6, high=1e6, dtype=np.float32, shape=(3 * H,))
            self.action_space = Box(low=-1e3, high=1e4, dtype=np.float32, shape=(1,))
            if mon is not None:
                from custom_envs_amd._native import MULTI_INFO_KEYS
                paths, mkw = mon
                if device_monitor:
                    mkw = dict(mkw, device=True)
                self.monitor = make_vec_monitor(E, paths, mkw, getattr(self._engine, 'device', 0))
                if self._device_monitor:
                    self.monitor.bind({key: ('info', c) for c, key in enumerate(MULTI_INFO_KEYS)},
                                      row_stride=P)
        else:
            runners = [functools.partial(OptEnvRunner, fn) for fn in environment_fns]
            self._host = ThreadVecEnv(runners)
            self.observation_space = self._host.observation_space
            self.action_space = self._host.action_space
            self.agent_no_list = self._host.get_attr('_num_agents')
        self.num_envs = sum(self.agent_no_list)

    @property
    def engine_backed(self):
        return self._engine is not None

    @property
    def _device_monitor(self):
        return getattr(self.monitor, 'on_device', False)

    def step_async(self, actions):
        if self._engine is not None and self.monitor is not None:
            self.monitor.check_step()
        self.waiting = True
        if self._engine is not None:
            self._engine.step_async(np.asarray(actions, np.float32).reshape(-1))
            return
        grouped, start = [], 0
        for n in self.agent_no_list:
            grouped.append(actions[start:start + n])
            start += n
        self._host.step_async(grouped)

    def step_wait(self):
        self.waiting = False
        if self._engine is not None:
            out = self._engine.step_wait()
            P = self._engine.n_params
            states = out['obs'].copy()
            rewards = out['reward'].copy()
            terminals = out['done'].astype(bool)
            env_rewards, env_dones = rewards[::P], terminals[::P]
            lengths = out['episode_len'].copy()
            info = out['info'].copy()
            episodes = {}
            infos = _RowInfos(info, env_rewards, env_dones, lengths, P, episodes)
            if self._device_monitor:
                episodes.update(self.monitor.step(env_rewards, env_dones, infos.per_env(),
                                                  fields={'info': info}))
            elif self.monitor is not None:
                episodes.update(self.monitor.step(env_rewards, env_dones, infos.per_env()))
                for env, ep in episodes.items():
                    infos.env_info(env)['episode'] = ep
        else:
            results = [remote.recv() for remote in self._host.remotes]
            self._host.waiting = False
            obs, rews, dones, infos = zip(*results)
            states = np.stack([o for group in obs for o in group])
            rewards = np.stack([r for group in rews for r in group])
            terminals = np.stack([d for group in dones for d in group])
            infos = [i for group in infos for i in group]
        for callback in self.callbacks:
            callback(states, rewards, terminals, infos)
        self._last_obs = states
        return states, rewards, terminals, infos

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def reset(self):
        if self._engine is not None:
            if self.monitor is not None:
                self.monitor.reset()
            self._last_obs = self._engine.reset()
            return self._last_obs
        groups = self._host._broadcast('reset', None)
        return np.stack([o for group in groups for o in group])

    def collect(self, policy, n_steps, noise=None, normalizer=None):
        """``n_steps`` closed-loop steps on the device as one engine call
        (``MultiOptEngine.rollout_policy``), one policy row per (env, agent)
        row, starting from the observation last returned; see
        ``GPUVecEnv.collect`` (``noise`` likewise: a tensor, None, False or a
        ``rng.DeviceRng``; ``normalizer`` likewise: the ``VecNormalize`` wrapped
        around this env).  Returns device tensors ``obs [K][rows][3H]``,
        ``actions``, ``env_actions``, ``values``, ``neglogps``, ``rewards``,
        ``dones``, ``last_obs``, ``last_values``, ``info [K][E][14]`` and
        ``episode_len``.  An attached monitor sees the K records in order
        afterwards; the step callbacks are not called.  The host path (envs
        that do not batch onto the engine) raises ``NotImplementedError``."""
        if self._engine is None:
            raise NotImplementedError('collect() needs the engine-backed OptVecEnv (every factory '
                                      'the same MultiOptLRs-v0 spec)')
        from custom_envs_amd.vectorize.collect import host_records, run_collect
        if self.monitor is not None:
            self.monitor.check_step()
        result, fields = run_collect(self._engine, policy, n_steps, self._last_obs, noise,
                                     self._engine.rows, normalizer)
        self._last_obs = fields['obs'][int(n_steps) - 1]     # the raw one
        if self._device_monitor:
            self.monitor.scan(fields, int(n_steps))
        elif self.monitor is not None:
            host, P = host_records(fields), self._engine.n_params
            for t in range(int(n_steps)):
                env_rewards, env_dones = host['reward'][t][::P], host['done'][t][::P].astype(bool)
                infos = _RowInfos(host['info'][t], env_rewards, env_dones, host['episode_len'][t],
                                  P, {})
                self.monitor.step(env_rewards, env_dones, infos.per_env())
        return result

    def collect_ddpg(self, agent, memory, n_steps, noise=None):
        """``n_steps`` closed-loop DDPG steps written straight into ``memory``
        (a ``custom_envs_amd.ddpg.ReplayMemory`` of one row per (env, agent)
        row per step); see ``GPUVecEnv.collect_ddpg``.  Returns device tensors
        ``env_actions [K][rows][1]``, ``info [K][E][14]``, ``episode_len`` and
        ``last_obs``.  An attached monitor sees the K records in order
        afterwards; the step callbacks are not called.  The host path raises
        ``NotImplementedError``; ``problem='nn'`` raises ``NativeEngineError``."""
        if self._engine is None:
            raise NotImplementedError('collect_ddpg() needs the engine-backed OptVecEnv (every '
                                      'factory the same MultiOptLRs-v0 spec)')
        import torch
        from custom_envs_amd._native import NativeEngineError
        from custom_envs_amd.multi_engine import NNMultiEngine
        from custom_envs_amd.vectorize.collect import run_collect_ddpg
        eng = self._engine
        if isinstance(eng, NNMultiEngine):
            raise NativeEngineError('the network problem has no K-step closed-loop form '
                                    '(DDPGAgent.act + step_device per step)')
        if self.monitor is not None:
            self.monitor.check_step()
        if getattr(self, '_ddpg_stream', None) is None:
            self._ddpg_stream = torch.cuda.Stream(torch.device('cuda', getattr(eng, 'device', 0)))
        keep = ('rewards', 'dones') if self.monitor is not None else ()
        result, kept = run_collect_ddpg(eng, agent, memory, n_steps, self._last_obs, noise,
                                        eng.rows, 3 * eng.max_history, 1, self._ddpg_stream, keep)
        self._last_obs = result['last_obs']
        if self._device_monitor:
            self.monitor.scan({'reward': kept['rewards'], 'done': kept['dones'],
                               'info': result['info']}, int(n_steps))
        elif self.monitor is not None:
            P = eng.n_params
            info, lengths = result['info'].cpu().numpy(), result['episode_len'].cpu().numpy()
            rewards, dones = kept['rewards'].cpu().numpy(), kept['dones'].cpu().numpy()
            for t in range(int(n_steps)):
                env_rewards, env_dones = rewards[t][::P], dones[t][::P].astype(bool)
                infos = _RowInfos(info[t], env_rewards, env_dones, lengths[t], P, {})
                self.monitor.step(env_rewards, env_dones, infos.per_env())
        return result

    def get_attr(self, attr_name, indices=None):
        if self._engine is None:
            return self._host.get_attr(attr_name, indices)
        E = self._engine.num_envs
        idx = range(E) if indices is None else ([indices] if isinstance(indices, int) else indices)
        if attr_name == '_num_agents':
            return [self._engine.n_params for _ in idx]
        if attr_name == 'current_step':
            step = self._engine.get_state()['step']
            return [int(step[i]) for i in idx]
        if attr_name in ('max_batches', 'max_history'):
            return [getattr(self._engine, attr_name) for _ in idx]
        raise AttributeError('engine-backed OptVecEnv has no per-env attribute %r' % attr_name)

    def env_method(self, method_name, *method_args, indices=None, **method_kwargs):
        if self._engine is None:
            return self._host.env_method(method_name, *method_args, indices=indices,
                                         **method_kwargs)
        monitor_methods = ('get_episode_rewards', 'get_episode_lengths', 'get_episode_times',
                           'get_total_steps')
        if method_name in monitor_methods and self.monitor is not None:
            return getattr(self.monitor, method_name)(indices)
        E = self._engine.num_envs
        idx = list(range(E)) if indices is None else (
            [indices] if isinstance(indices, int) else list(indices))
        if method_name == 'seed':
            # BaseEnvironment.seed per env (baseenvironment.py:20-28); the
            # 'nn' problem draws its weights and shuffles from these seeds
            from custom_envs_amd.engine import normalize_seed
            seed = method_args[0] if method_args else method_kwargs.get('seed')
            # env i's seed changes only for i in indices: the others keep the
            # engine's current seeds, however they were set
            seeds = list(getattr(self._engine, 'seeds', None) or getattr(self, '_seeds', range(E)))
            for i in idx:
                seeds[i] = normalize_seed(seed)
            self._engine.seed(seeds)
            self._seeds = seeds
            return [[seeds[i]] for i in idx]
        if method_name == 'render':
            return [None] * len(idx)
        raise AttributeError('engine-backed OptVecEnv has no per-env method %r' % method_name)

    def render(self, *args, **kwargs):
        return None

    def close(self):
        if self.closed:
            return
        self.closed = True
        if self._engine is not None:
            if self.monitor is not None:
                self.monitor.close()
            self._engine.close()
        else:
            self._host.close()

