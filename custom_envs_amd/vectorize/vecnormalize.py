"""``VecNormalize``: stable-baselines' running observation / return scaling
on the device.

stable-baselines 2.x wraps a ``VecEnv`` in ``VecNormalize`` so a learner sees
observations with zero mean and unit variance per column and rewards divided by
the standard deviation of the discounted return, both clipped.  Here the
statistics live on the device and one kernel launch does one step
(``csrc/vecnorm_kernels.h``), so ``collect`` stays one foreign call:
``[policy, env step, normalise] x K`` (``ce_rollout_policy_vecnorm``), the
policy reading the normalised observation of the step before.

``vecnormalize_numpy`` states the semantics in NumPy (float64), written as
remembered from stable-baselines 2.x, which is not installed where this was
written, so it was not compared against it.

What differs from stable-baselines, on purpose:

* ``venv`` is a ``GPUVecEnv`` or an engine-backed ``OptVecEnv``; rows are envs
  x agents and the statistics run per column over all rows.
* ``save_running_average`` / ``load_running_average`` use one ``.npz`` without
  pickle, not SB's two pickles, and include ``ret``: a resumed run continues
  bit for bit.
* ``collect_ddpg`` (and so ``DDPG``), ``distribute`` and the network problem's
  engine raise.
* Whether normalisation improves learning on these envs has not been measured.
"""
import ctypes
import os

import numpy as np

from custom_envs_amd import _native

STATE_KEYS = ('obs_mean', 'obs_var', 'obs_count', 'ret_mean', 'ret_var', 'ret_count', 'ret')
FILE_NAME = 'vecnormalize.npz'
MAX_ROWS, MAX_OBS_DIM = 1 << 24, 1 << 16


# ------------------------------------------------------------- the statement
def initial_state(rows, obs_dim):
    """mean 0, variance 1, count 1e-4 (SB's ``RunningMeanStd``), ``ret`` 0."""
    return {'obs_mean': np.zeros(obs_dim), 'obs_var': np.ones(obs_dim), 'obs_count': 1e-4,
            'ret_mean': 0.0, 'ret_var': 1.0, 'ret_count': 1e-4, 'ret': np.zeros(rows)}


def update_numpy(mean, var, count, x):
    """``RunningMeanStd.update``: the moments merged with the batch ``x``
    (rows first; float64).  Returns (mean, var, count)."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    bm = x.mean(axis=0)
    bv = ((x - bm) ** 2).mean(axis=0)          # population, two-pass
    d = bm - mean
    tot = count + n
    new_mean = mean + d * n / tot
    new_var = (var * count + bv * n + d * d * count * n / tot) / tot
    return new_mean, new_var, tot


def vecnormalize_numpy(state, obs, reward=None, done=None, training=True, norm_obs=True,
                       norm_reward=True, clip_obs=10.0, clip_reward=10.0, gamma=0.99,
                       epsilon=1e-8, reset=False):
    """One ``VecNormalize.step_wait`` (``reset``: ``VecNormalize.reset``) on
    ``state`` (``initial_state``; changed in place): ``obs`` float32
    ``[rows][D]``, ``reward`` float32 ``[rows]``, ``done`` ``[rows]``.  Returns
    (normalised obs float32, normalised reward float32 or None for a reset).

        if training and norm_obs:    obs moments = update(obs moments, obs)
        obs_n = f32(clip((obs - mean) / sqrt(var + epsilon), +-clip_obs))
        ret = ret * gamma + reward
        if training and norm_reward: ret moments = update(ret moments, ret)
        rew_n = f32(clip(reward / sqrt(ret var + epsilon), +-clip_reward))
        ret[done] = 0

    A reset clears ``ret``, updates the obs moments as a step does and leaves
    the return moments alone.  With a switch off that output is the input."""
    obs = np.asarray(obs, np.float32)
    x = obs.astype(np.float64)
    if norm_obs:
        if training:
            state['obs_mean'], state['obs_var'], state['obs_count'] = update_numpy(
                state['obs_mean'], state['obs_var'], state['obs_count'], x)
        obs_n = np.clip((x - state['obs_mean']) / np.sqrt(state['obs_var'] + epsilon),
                        -clip_obs, clip_obs).astype(np.float32)
    else:
        obs_n = obs.copy()
    if reset:
        state['ret'] = np.zeros_like(state['ret'])
        return obs_n, None
    reward = np.asarray(reward, np.float32)
    state['ret'] = state['ret'] * gamma + reward.astype(np.float64)
    if norm_reward:
        if training:
            state['ret_mean'], state['ret_var'], state['ret_count'] = (float(v) for v in update_numpy(
                state['ret_mean'], state['ret_var'], state['ret_count'], state['ret']))
        rew_n = np.clip(reward.astype(np.float64) / np.sqrt(state['ret_var'] + epsilon),
                        -clip_reward, clip_reward).astype(np.float32)
    else:
        rew_n = reward.copy()
    state['ret'] = np.where(np.asarray(done).astype(bool), 0.0, state['ret'])
    return obs_n, rew_n


# ------------------------------------------------------------ the device side
def check_config(rows, obs_dim, clip_obs, clip_reward, gamma, epsilon):
    """What ``ce_vecnorm_create`` refuses, as ``ValueError`` (no GPU)."""
    if not 1 <= int(rows) <= MAX_ROWS:
        raise ValueError('rows must be in [1, 2^24], got %d' % rows)
    if not 1 <= int(obs_dim) <= MAX_OBS_DIM:
        raise ValueError('obs_dim must be in [1, 2^16], got %d' % obs_dim)
    if not (float(clip_obs) > 0 and float(clip_reward) > 0):
        raise ValueError('clip_obs and clip_reward must be positive')
    if not np.isfinite(float(gamma)):
        raise ValueError('gamma must be finite')
    if not (np.isfinite(float(epsilon)) and float(epsilon) >= 0):
        raise ValueError('epsilon must be finite and not negative')


def slot_floats(rows, obs_dim):
    """Floats between the normalised observation slots of a rollout: rows *
    obs_dim rounded up to a multiple of 4 (the slots are 16-byte aligned)."""
    return -(-int(rows) * int(obs_dim) // 4) * 4


class NormalizedRollout:
    """The normalised side of one ``rollout_policy`` call: ``obs``
    ``[k + 1][rows][D]`` (slot 0 the observation the rollout starts from, slot
    ``s + 1`` what step ``s`` produced) and ``rewards`` ``[k][rows]``."""

    def __init__(self, normalizer, k, obs, rewards, training):
        self.normalizer, self.k, self.obs, self.rewards = normalizer, int(k), obs, rewards
        self.training = bool(training)


def check_normalized_rollout(roll, k, rows, obs_dim, device):
    """Every check of the normalised buffers of a rollout before a pointer
    reaches C (no GPU up to the device checks, which come last).  Returns
    (obs step bytes, reward step bytes)."""
    import torch
    if not isinstance(roll, NormalizedRollout):
        raise TypeError('normalizer must be a NormalizedRollout (DeviceVecNorm.begin_rollout)')
    vn = roll.normalizer
    if (vn.rows, vn.obs_dim) != (rows, obs_dim):
        raise ValueError('the normaliser holds %d rows of %d columns, the engine\'s rows are %d of %d'
                         % (vn.rows, vn.obs_dim, rows, obs_dim))
    if vn.device != device:
        raise ValueError('the normaliser lives on cuda:%d, the engine on cuda:%d'
                         % (vn.device, device))
    for name, t, need, tail in (('obs', roll.obs, k + 1, (rows, obs_dim)),
                                ('rewards', roll.rewards, k, (rows,))):
        if t.dtype != torch.float32:
            raise ValueError('normalised %s must have dtype float32, got %s' % (name, t.dtype))
        if tuple(t.shape[1:]) != tail:
            raise ValueError('normalised %s records have shape %s, the call writes %s'
                             % (name, tuple(t.shape[1:]), tail))
        if t.shape[0] < need:
            raise ValueError('normalised %s holds %d records, the call needs %d'
                             % (name, t.shape[0], need))
        if not t[0].is_contiguous():
            raise ValueError('normalised %s: every record must be contiguous' % name)
        step = t.stride(0) * 4
        if step % 16 or step < int(np.prod(tail)) * 4:
            raise ValueError('normalised %s: the record stride (%d B) must be a multiple of 16 of '
                             'at least the record\'s bytes' % (name, step))
    for name, t in (('obs', roll.obs), ('rewards', roll.rewards)):
        if t.device.type != 'cuda' or t.device.index != device:
            raise ValueError('normalised %s must be on device cuda:%d, got %s'
                             % (name, device, t.device))
    if roll.obs.data_ptr() % 16:
        raise ValueError('normalised obs must be 16-byte aligned')
    return roll.obs.stride(0) * 4, roll.rewards.stride(0) * 4


def noise_struct(noise, stride):
    """``ce_rollout_noise`` of a rollout's noise: a tensor (``stride`` elements
    between steps), None, or a ``DeviceRng``."""
    if hasattr(noise, 'row_offset'):
        return _native.CeRolloutNoise(kind=_native.CE_NOISE_GENERATED, seed=noise.seed,
                                      t0=int(noise.t), row0=noise.row_offset)
    return _native.CeRolloutNoise(kind=_native.CE_NOISE_BLOCK,
                                  ptr=None if noise is None else noise.data_ptr(),
                                  stride=int(stride))


def rollout_call(fn, name, handle, policy, roll, k, rows, obs_dim, act_dim, device, noise, outputs,
                 record_bytes, policy_outputs, policy_record_bytes):
    """The normalised form of an engine's ``rollout_policy``: validates
    ``roll`` and calls ``ce_*rollout_policy_vecnorm`` (``fn``)."""
    obs_step, rew_step = check_normalized_rollout(roll, int(k), rows, obs_dim, device)
    ns = noise_struct(noise, rows * act_dim)
    flags = _native.CE_VECNORM_TRAINING if roll.training else 0
    _native.check(fn(handle, policy._h, roll.normalizer._h, int(k), roll.obs.data_ptr(), obs_step,
                     roll.rewards.data_ptr(), rew_step, flags, ctypes.byref(ns),
                     ctypes.byref(outputs), int(record_bytes), ctypes.byref(policy_outputs),
                     int(policy_record_bytes)), name)


class DeviceVecNorm:
    """Handle on one ``ce_vecnorm``: the running moments and ``ret`` on the
    device, and the current observation (raw and normalised) and reward as
    device tensors."""

    def __init__(self, rows, obs_dim, norm_obs=True, norm_reward=True, clip_obs=10.0,
                 clip_reward=10.0, gamma=0.99, epsilon=1e-8, device=0):
        check_config(rows, obs_dim, clip_obs, clip_reward, gamma, epsilon)
        lib = _native.load()
        self.rows, self.obs_dim, self.device = int(rows), int(obs_dim), int(device)
        cfg = _native.CeVecnormConfig(abi_version=_native.ABI_VERSION, device=self.device,
                                      rows=self.rows, obs_dim=self.obs_dim,
                                      norm_obs=1 if norm_obs else 0,
                                      norm_reward=1 if norm_reward else 0,
                                      clip_obs=float(clip_obs), clip_reward=float(clip_reward),
                                      gamma=float(gamma), epsilon=float(epsilon))
        handle = ctypes.c_void_p()
        _native.check(lib.ce_vecnorm_create(ctypes.byref(cfg), ctypes.byref(handle)),
                      'ce_vecnorm_create')
        self._lib, self._h = lib, handle
        self.obs = self.original_obs = self.original_reward = self.reward = None

    @staticmethod
    def _stream(stream):
        if stream is not None:
            return ctypes.c_void_p(stream or 0)
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream or 0)

    def _check(self, name, t, dtype, shape):
        if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise ValueError('%s must be a contiguous %s tensor of shape %s, got %s %s'
                             % (name, dtype, tuple(shape), t.dtype, tuple(t.shape)))
        if t.device.type != 'cuda' or t.device.index != self.device:
            raise ValueError('%s must be on device cuda:%d, got %s' % (name, self.device, t.device))

    def step_device(self, obs, reward=None, done=None, training=True, reset=False, obs_only=False,
                    obs_out=None, reward_out=None, stream=None):
        """One launch on ``stream`` (default: torch's current stream) over
        device tensors: ``obs`` ``[rows][D]`` float32, ``reward`` ``[rows]``
        float32, ``done`` ``[rows]`` uint8.  ``reset``: ``VecNormalize.reset``
        (no reward).  ``obs_only``: normalise ``obs`` and touch nothing else.
        Returns (normalised obs, normalised reward or None)."""
        import torch
        self._check('obs', obs, torch.float32, (self.rows, self.obs_dim))
        if obs_out is None:
            obs_out = torch.empty_like(obs)
        self._check('obs_out', obs_out, torch.float32, (self.rows, self.obs_dim))
        flags = _native.CE_VECNORM_TRAINING if training and not obs_only else 0
        if reset or obs_only:
            flags |= _native.CE_VECNORM_RESET if reset else _native.CE_VECNORM_OBS_ONLY
            reward = done = reward_out = None
        else:
            self._check('reward', reward, torch.float32, (self.rows,))
            self._check('done', done, torch.uint8, (self.rows,))
            if reward_out is None:
                reward_out = torch.empty_like(reward)
            self._check('reward_out', reward_out, torch.float32, (self.rows,))
        ptr = lambda t: None if t is None else t.data_ptr()
        _native.check(self._lib.ce_vecnorm_step(self._h, ptr(obs), ptr(reward), ptr(done),
                                                ptr(obs_out), ptr(reward_out), flags,
                                                self._stream(stream)), 'ce_vecnorm_step')
        return obs_out, reward_out

    def begin_rollout(self, k, training):
        """The normalised buffers of a K-step rollout, slot 0 holding the
        current normalised observation."""
        import torch
        if self.obs is None:
            raise RuntimeError('the normaliser has no observation to start from: call reset() on '
                               'the VecNormalize wrapper first')
        k = int(k)
        dev = torch.device('cuda', self.device)
        sf = slot_floats(self.rows, self.obs_dim)
        rf = slot_floats(self.rows, 1)
        obs = torch.zeros((k + 1) * sf, dtype=torch.float32, device=dev).as_strided(
            (k + 1, self.rows, self.obs_dim), (sf, self.obs_dim, 1))
        rewards = torch.zeros(k * rf, dtype=torch.float32, device=dev).as_strided(
            (k, self.rows), (rf, 1))
        obs[0].copy_(self.obs)
        return NormalizedRollout(self, k, obs, rewards, training)

    def end_rollout(self, roll, raw_obs, raw_reward):
        """Keep what the rollout's last step produced as the current values."""
        k = roll.k
        self.obs = roll.obs[k].clone()
        self.reward = roll.rewards[k - 1].clone()
        self.original_obs, self.original_reward = raw_obs.clone(), raw_reward.clone()

    def get_state(self):
        """The seven entries of ``initial_state`` from the device (synchronises)."""
        st = {'obs_mean': np.zeros(self.obs_dim), 'obs_var': np.zeros(self.obs_dim),
              'obs_count': np.zeros(1), 'ret_mean': np.zeros(1), 'ret_var': np.zeros(1),
              'ret_count': np.zeros(1), 'ret': np.zeros(self.rows)}
        _native.check(self._lib.ce_vecnorm_get_state(
            self._h, *(st[k].ctypes.data for k in STATE_KEYS), self._stream(None)),
            'ce_vecnorm_get_state')
        return {k: (v if k in ('obs_mean', 'obs_var', 'ret') else float(v[0]))
                for k, v in st.items()}

    def set_state(self, state):
        shapes = {'obs_mean': (self.obs_dim,), 'obs_var': (self.obs_dim,), 'ret': (self.rows,)}
        arrays = {}
        for key in STATE_KEYS:
            if key not in state:
                raise ValueError('the state lacks %r' % key)
            a = np.ascontiguousarray(state[key], np.float64).reshape(-1)
            want = shapes.get(key, (1,))
            if a.shape != want:
                raise ValueError('state %s must have shape %s, got %s' % (key, want, a.shape))
            arrays[key] = a
        _native.check(self._lib.ce_vecnorm_set_state(
            self._h, *(arrays[k].ctypes.data for k in STATE_KEYS), self._stream(None)),
            'ce_vecnorm_set_state')

    def close(self):
        if getattr(self, '_h', None):
            self._lib.ce_vecnorm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def wrapped_shape(venv):
    """(engine, rows, obs_dim, device) of an env ``VecNormalize`` can wrap;
    anything else: ``TypeError``; the network problem: ``NotImplementedError``."""
    from custom_envs_amd.vectorize.gpuvecenv import GPUVecEnv
    from custom_envs_amd.vectorize.optvecenv import OptVecEnv
    if isinstance(venv, GPUVecEnv):
        eng = venv.engine
        return eng, venv.num_envs, eng.obs_dim, eng.device
    if isinstance(venv, OptVecEnv) and venv.engine_backed:
        from custom_envs_amd.multi_engine import NNMultiEngine
        eng = venv._engine
        if isinstance(eng, NNMultiEngine):
            raise NotImplementedError('VecNormalize does not wrap the network problem: its engine '
                                      'has no rollout_policy')
        return eng, eng.rows, 3 * eng.max_history, getattr(eng, 'device', 0)
    raise TypeError('VecNormalize wraps a GPUVecEnv or an engine-backed OptVecEnv (every factory '
                    'the same MultiOptLRs-v0 spec), got %s' % type(venv).__name__)


class VecNormalize:
    """stable-baselines' ``VecNormalize`` over a ``GPUVecEnv`` or an
    engine-backed ``OptVecEnv`` (see the module docstring).  ``reset``,
    ``step_wait`` and ``collect`` run the same device kernel on one state.
    ``training`` may be switched at any time (False: the moments stay as they
    are, as for evaluation)."""

    def __init__(self, venv, training=True, norm_obs=True, norm_reward=True, clip_obs=10.,
                 clip_reward=10., gamma=0.99, epsilon=1e-8):
        _, rows, obs_dim, device = wrapped_shape(venv)
        self.venv = venv
        self.training = bool(training)
        self.norm_obs, self.norm_reward = bool(norm_obs), bool(norm_reward)
        self.clip_obs, self.clip_reward = float(clip_obs), float(clip_reward)
        self.gamma, self.epsilon = float(gamma), float(epsilon)
        self.normalizer = DeviceVecNorm(rows, obs_dim, norm_obs, norm_reward, clip_obs,
                                        clip_reward, gamma, epsilon, device)
        self.closed = False

    # ------------------------------------------------------------- forwarding
    num_envs = property(lambda self: self.venv.num_envs)
    observation_space = property(lambda self: self.venv.observation_space)
    action_space = property(lambda self: self.venv.action_space)
    monitor = property(lambda self: self.venv.monitor)
    unwrapped = property(lambda self: self.venv)

    def __getattr__(self, name):
        if name.startswith('_') or name == 'venv':
            raise AttributeError(name)
        return getattr(self.venv, name)          # agent_no_list, waiting, ...

    def env_method(self, method_name, *method_args, indices=None, **method_kwargs):
        return self.venv.env_method(method_name, *method_args, indices=indices, **method_kwargs)

    def get_attr(self, attr_name, indices=None):
        return self.venv.get_attr(attr_name, indices)

    def seed(self, seed=None):
        if hasattr(self.venv, 'seed'):
            return self.venv.seed(seed)
        return self.venv.env_method('seed', seed)

    def close(self):
        if not self.closed:
            self.closed = True
            self.normalizer.close()
            self.venv.close()

    def __len__(self):
        return self.num_envs

    # ------------------------------------------------------------- VecEnv API
    def _upload(self, array, dtype):
        import torch
        t = torch.from_numpy(np.ascontiguousarray(array, dtype=dtype))
        return t.to(torch.device('cuda', self.normalizer.device))

    def reset(self):
        import torch
        vn = self.normalizer
        raw = self._upload(self.venv.reset(), np.float32).reshape(vn.rows, vn.obs_dim)
        vn.obs, _ = vn.step_device(raw, training=self.training, reset=True)
        vn.original_obs, vn.original_reward, vn.reward = raw, None, None
        torch.cuda.current_stream(raw.device).synchronize()
        return vn.obs.cpu().numpy()

    def step_async(self, actions):
        self.venv.step_async(actions)

    def step_wait(self):
        import torch
        vn = self.normalizer
        obs, rewards, dones, infos = self.venv.step_wait()
        raw = self._upload(obs, np.float32).reshape(vn.rows, vn.obs_dim)
        rew = self._upload(rewards, np.float32).reshape(vn.rows)
        done = self._upload(np.asarray(dones).astype(np.uint8), np.uint8).reshape(vn.rows)
        vn.obs, vn.reward = vn.step_device(raw, rew, done, training=self.training)
        vn.original_obs, vn.original_reward = raw, rew
        torch.cuda.current_stream(raw.device).synchronize()
        return vn.obs.cpu().numpy(), vn.reward.cpu().numpy(), dones, infos

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def get_original_obs(self):
        """The last raw observation (numpy), as the wrapped env returned it."""
        t = self.normalizer.original_obs
        return None if t is None else t.cpu().numpy()

    def get_original_reward(self):
        t = self.normalizer.original_reward
        return None if t is None else t.cpu().numpy()

    @property
    def _last_obs(self):
        """The normalised observation ``collect`` starts from (None before the
        first reset).  A wrapper put around an env that already has an
        observation (a resumed run) normalises that one with the moments as
        they are, touching neither them nor ``ret``."""
        import torch
        vn = self.normalizer
        if vn.obs is None:
            raw = getattr(self.venv, '_last_obs', None)
            if raw is None:
                return None
            if not torch.is_tensor(raw):
                raw = self._upload(raw, np.float32)
            raw = raw.to(torch.device('cuda', vn.device)).reshape(vn.rows, vn.obs_dim).contiguous()
            vn.obs, _ = vn.step_device(raw, obs_only=True)
            vn.original_obs = raw.clone()
            torch.cuda.current_stream(raw.device).synchronize()
        return vn.obs

    def collect(self, policy, n_steps, noise=None):
        """The wrapped env's ``collect`` with the normaliser inside the
        rollout: ``obs``, ``last_obs`` and ``rewards`` are normalised,
        ``last_values`` comes from the normalised last observation, and the raw
        values are added as ``original_obs`` and ``original_rewards``.  An
        attached monitor keeps seeing the raw rewards."""
        if self._last_obs is None:
            raise RuntimeError('collect() needs an observation to start from: call reset() first')
        return self.venv.collect(policy, n_steps, noise, normalizer=self)

    def collect_ddpg(self, *args, **kwargs):
        raise NotImplementedError('collect_ddpg() on a VecNormalize env is not supported: DDPG '
                                  'normalises inside its own graph in stable-baselines')

    # -------------------------------------------------------- running average
    def save_running_average(self, path):
        """The moments and ``ret`` as ``<path>/vecnormalize.npz`` (``np.savez``,
        no pickle)."""
        np.savez(os.path.join(str(path), FILE_NAME), **self.normalizer.get_state())

    def load_running_average(self, path):
        """What ``save_running_average`` wrote.  stable-baselines' own pickles
        (``obs_rms.pkl`` / ``ret_rms.pkl``) are not read."""
        file = os.path.join(str(path), FILE_NAME)
        if not os.path.exists(file):
            if os.path.exists(os.path.join(str(path), 'obs_rms.pkl')):
                raise NotImplementedError('stable-baselines\' pickled running averages are not '
                                          'read: save them with save_running_average')
            raise FileNotFoundError(file)
        with np.load(file, allow_pickle=False) as data:
            self.normalizer.set_state({k: data[k] for k in STATE_KEYS})
