"""Episode logging: the scripts' ``Monitor`` and a vectorised ``VecMonitor``.

``Monitor`` keeps the reference's constructor and behaviour
(custom_envs/utils/utils_logging.py:15-156): callbacks fed every step,
episode rows ``r, l, t, current_reward, episode`` plus ``info_keywords``
appended on done and written in ``chunk_size`` chunks to ``<path>.mon.csv``
with sorted columns.  Two reference bugs are not reproduced:
``get_total_steps`` counts steps (the reference reads an attribute it never
sets) and ``get_episode_times`` returns times (the reference returns rewards).

``VecMonitor`` does the same bookkeeping for a whole engine-backed vector env
from its batched reward/done arrays, so monitored envs do not put a Python
wrapper call per env per step back on the hot path.

``DeviceVecMonitor`` is ``VecMonitor`` with that bookkeeping as HIP kernels over
the rollout records where ``collect`` left them (``ce_monitor_*``,
csrc/monitor_kernels.h; opt-in through the vec envs): only the finished
episodes' records come to the host.  ``episodes_numpy`` and
``explained_variance_numpy`` state its kernels in NumPy.
"""
import time
from collections import defaultdict
from pathlib import Path

import numpy as np

from custom_envs_amd.core import Wrapper

EXT = '.mon.csv'


def _mon_path(file_path):
    return None if file_path is None else Path(file_path).resolve().with_suffix(EXT)


def _save_rows(path, rows):
    if path is None or not rows:
        return
    import pandas as pd
    header = not path.is_file()
    frame = pd.DataFrame(rows)
    frame = frame.reindex(sorted(frame.columns), axis=1)
    frame.to_csv(path, header=header, index=False, mode='w' if header else 'a')


class Monitor(Wrapper):
    """utils_logging.Monitor: wraps one env (or an env factory)."""
    EXT = EXT

    def __init__(self, env, file_path, info_keywords=(), chunk_size=1, callbacks=None,
                 allow_early_resets=True):
        if callable(env) and not hasattr(env, 'step'):
            env = env()
        super().__init__(env)
        self.t_start = time.time()
        self.file_path = _mon_path(file_path)
        self.chunk_size = chunk_size
        self.info_keywords = info_keywords
        self.allow_early_resets = allow_early_resets
        self.last_info = {}
        self.rewards = None
        self.metric_history = defaultdict(list)
        self.current_episode = 0
        self.callbacks = [] if callbacks is None else callbacks
        self.data = []
        self.total_steps = 0

    def save(self):
        _save_rows(self.file_path, self.data)
        self.data = []

    def reset(self, **kwargs):
        self.rewards = []
        self.current_episode += 1
        return self.env.reset(**kwargs)

    def step(self, action):
        observation, reward, done, info = self.env.step(action)
        for callback in self.callbacks:
            callback({'observation': observation, 'reward': reward, 'done': done,
                      'info': info, 'episode': self.current_episode})
        self.rewards.append(reward)
        self.total_steps += 1
        if done:
            ep_rew = sum(self.rewards)
            ep_info = {'r': round(ep_rew, 6), 'l': len(self.rewards),
                       't': round(time.time() - self.t_start, 6),
                       'current_reward': reward, 'episode': self.current_episode}
            self.last_info = info
            for key in self.info_keywords:
                ep_info[key] = info[key]
            self.data.append(ep_info)
            if len(self.data) >= self.chunk_size:
                self.save()
            info['episode'] = ep_info
            self.metric_history['rewards'].append(ep_rew)
            self.metric_history['lengths'].append(len(self.rewards))
            self.metric_history['times'].append(time.time() - self.t_start)
        return observation, reward, done, info

    def close(self):
        if self.data:
            self.save()
        return self.env.close()

    def get_total_steps(self):
        return self.total_steps

    def get_episode_rewards(self):
        return self.metric_history.get('rewards', [])

    def get_episode_lengths(self):
        return self.metric_history.get('lengths', [])

    def get_episode_times(self):
        return self.metric_history.get('times', [])


class VecMonitor:
    """Monitor bookkeeping for E envs at once (one row of arrays per step).

    ``file_paths`` is one path (or None) per env, as the per-env Monitors of
    the reference had; ``step`` takes per-env rewards, dones and an info
    sequence and returns the per-env episode dicts of envs that finished.
    ``style``: 'logging' writes utils_logging.Monitor's rows (r, l, t,
    current_reward, episode + info_keywords; utils_logging.py:98-116),
    'sb' the stable-baselines wrappers.monitor.Monitor's (r, l, t +
    info_keywords, monitor.py:94-123), whose reset refuses envs still in an
    episode unless ``allow_early_resets`` (monitor.py:69-75).
    """

    def __init__(self, num_envs, file_paths=None, info_keywords=(), chunk_size=1,
                 callbacks=None, style='logging', allow_early_resets=True,
                 reset_keywords=()):
        if style not in ('logging', 'sb'):
            raise ValueError('style must be logging or sb')
        self.style = style
        self.reset_keywords = tuple(reset_keywords or ())
        if self.reset_keywords and style != 'sb':
            raise ValueError('reset_keywords belong to the sb style')
        self.allow_early_resets = bool(allow_early_resets)
        self.needs_reset = np.ones(num_envs, bool)
        self.num_envs = num_envs
        if file_paths is None or isinstance(file_paths, (str, Path)):
            file_paths = [file_paths] * num_envs if file_paths is None else [
                '%s_%d' % (file_paths, i) for i in range(num_envs)]
        self.paths = [_mon_path(p) for p in file_paths]
        self.info_keywords = tuple(info_keywords)
        self.chunk_size = chunk_size
        self.callbacks = list(callbacks or ())
        self.t_start = time.time()
        self.ep_reward = np.zeros(num_envs)
        self.ep_len = np.zeros(num_envs, np.int64)
        self.current_episode = np.zeros(num_envs, np.int64)
        self.data = [[] for _ in range(num_envs)]
        self.metric_history = [defaultdict(list) for _ in range(num_envs)]
        self.total_steps = np.zeros(num_envs, np.int64)
        # per env, as each reference Monitor keeps its own current_reset_info
        # (monitor.py:84-90): a partial reset stamps only the envs it resets
        self.reset_info = [{} for _ in range(num_envs)]

    def reset(self, indices=None, **kwargs):
        idx = slice(None) if indices is None else indices
        if self.style == 'sb' and not self.allow_early_resets and not self.needs_reset[idx].all():
            raise RuntimeError('Tried to reset an environment before done. If you want to '
                               'allow early resets, wrap your env with Monitor(env, path, '
                               'allow_early_resets=True)')
        self.needs_reset[idx] = False         # before the keyword check, monitor.py:84-85
        for key in self.reset_keywords:
            if kwargs.get(key) is None:
                raise ValueError('Expected you to pass kwarg %s into reset' % key)
        envs = range(len(self.reset_info)) if indices is None else np.arange(
            len(self.reset_info))[indices]
        for i in np.atleast_1d(envs):
            for key in self.reset_keywords:
                self.reset_info[int(i)][key] = kwargs[key]
        self.ep_reward[idx] = 0.0
        self.ep_len[idx] = 0
        self.current_episode[idx] += 1

    def check_step(self):
        """Called before the engine launches a step: the SB Monitor refuses
        to step an env that needs a reset (monitor.py:87-88)."""
        if self.style == 'sb' and self.needs_reset.any():
            raise RuntimeError('Tried to step environment that needs reset')

    def step(self, rewards, dones, infos, observations=None):
        rewards = np.asarray(rewards, dtype=np.float64)
        dones = np.asarray(dones, dtype=bool)
        if self.callbacks:
            for i in range(self.num_envs):
                payload = {'observation': None if observations is None else observations[i],
                           'reward': float(rewards[i]), 'done': bool(dones[i]),
                           'info': infos[i], 'episode': int(self.current_episode[i])}
                for callback in self.callbacks:
                    callback(payload)
        self.ep_reward += rewards
        self.ep_len += 1
        self.total_steps += 1
        finished = {}
        now = time.time() - self.t_start
        for i in np.flatnonzero(dones):
            info = infos[i]
            self.needs_reset[i] = True
            ep_info = {'r': round(float(self.ep_reward[i]), 6), 'l': int(self.ep_len[i]),
                       't': round(now, 6)}
            if self.style == 'logging':
                ep_info['current_reward'] = float(rewards[i])
                ep_info['episode'] = int(self.current_episode[i])
            for key in self.info_keywords:
                ep_info[key] = info[key]
            ep_info.update(self.reset_info[i])
            self.data[i].append(ep_info)
            if len(self.data[i]) >= self.chunk_size:
                _save_rows(self.paths[i], self.data[i])
                self.data[i] = []
            history = self.metric_history[i]
            history['rewards'].append(float(self.ep_reward[i]))
            history['lengths'].append(int(self.ep_len[i]))
            history['times'].append(now)
            finished[int(i)] = ep_info
        if finished:   # auto-reset happened in the engine: the Monitor's reset()
            self.reset(list(finished))
        return finished

    def close(self):
        for i in range(self.num_envs):
            _save_rows(self.paths[i], self.data[i])
            self.data[i] = []

    def get_episode_rewards(self, indices=None):
        idx = range(self.num_envs) if indices is None else indices
        return [self.metric_history[i].get('rewards', []) for i in idx]

    def get_episode_lengths(self, indices=None):
        idx = range(self.num_envs) if indices is None else indices
        return [self.metric_history[i].get('lengths', []) for i in idx]

    def get_episode_times(self, indices=None):
        idx = range(self.num_envs) if indices is None else indices
        return [self.metric_history[i].get('times', []) for i in idx]

    def get_total_steps(self, indices=None):
        idx = range(self.num_envs) if indices is None else indices
        return [int(self.total_steps[i]) for i in idx]


# ------------------------------------------------------- the device monitor
def record_dtype(n_info):
    """One episode record as the write kernel lays it out
    (``ce_monitor_record_bytes``): env, t, r (the float64 sum, unrounded), l,
    current_reward, episode and ``n_info`` float32 info columns, padded to a
    multiple of 8 bytes."""
    n_info = int(n_info)
    names = ['env', 't', 'r', 'l', 'current_reward', 'episode']
    formats = ['<i4', '<i4', '<f8', '<i4', '<f4', '<i8']
    offsets = [0, 4, 8, 16, 20, 24]
    if n_info:
        names.append('info')
        formats.append(('<f4', (n_info,)))
        offsets.append(32)
    return np.dtype({'names': names, 'formats': formats, 'offsets': offsets,
                     'itemsize': 32 + 8 * ((n_info + 1) // 2)})


def new_carry(num_envs):
    """What the monitor carries from one call to the next, per env."""
    return {'ep_reward': np.zeros(num_envs, np.float64), 'ep_len': np.zeros(num_envs, np.int32),
            'episode': np.zeros(num_envs, np.int64), 'total_steps': np.zeros(num_envs, np.int64)}


def episodes_numpy(rewards, dones, info=None, carry=None):
    """The statement of the device monitor's scan and of its record order (no
    GPU): ``VecMonitor.step`` over ``rewards`` / ``dones`` ``[K][E]`` (float32
    / any integer or bool) and the selected info columns ``info [K][E][n]``
    (float32, or None), starting from ``carry`` (``new_carry``; None: zeros).
    Per step, in ``VecMonitor.step``'s order: ``ep_reward += float64(reward)``,
    ``ep_len += 1``; an env whose done is set gives one record, then its sums
    are cleared and its episode number advances.  Returns (records, a
    ``record_dtype`` array in (t, env) order; the new carry).  ``l`` is the
    monitor's own count, as ``VecMonitor``'s, so the engines' ``episode_len``
    field is not an input."""
    rewards = np.asarray(rewards, np.float32)
    if rewards.ndim != 2:
        raise ValueError('rewards must have shape [K][E], got %s' % (rewards.shape,))
    K, E = rewards.shape
    dones = np.asarray(dones) != 0
    if dones.shape != (K, E):
        raise ValueError('dones must have shape %s, got %s' % ((K, E), dones.shape))
    n_info = 0
    if info is not None:
        info = np.asarray(info, np.float32)
        if info.ndim != 3 or info.shape[:2] != (K, E):
            raise ValueError('info must have shape [%d][%d][n], got %s' % (K, E, info.shape))
        n_info = info.shape[2]
    carry = new_carry(E) if carry is None else {k: np.array(v) for k, v in carry.items()}
    ep_reward, ep_len = carry['ep_reward'], carry['ep_len']
    rows = []
    for t in range(K):
        ep_reward += rewards[t].astype(np.float64)
        ep_len += 1
        for e in np.flatnonzero(dones[t]):
            rows.append((e, t, ep_reward[e], ep_len[e], rewards[t, e], carry['episode'][e])
                        + ((info[t, e],) if n_info else ()))
            ep_reward[e] = 0.0
            ep_len[e] = 0
            carry['episode'][e] += 1
    carry['total_steps'] += K
    records = np.zeros(len(rows), record_dtype(n_info))
    for i, row in enumerate(rows):
        records[i] = row
    return records, carry


def explained_variance_numpy(values, returns):
    """stable-baselines' ``explained_variance(y_pred, y)`` in float64: ``1 -
    Var[returns - values] / Var[returns]`` over every entry (population
    variances); NaN when ``Var[returns] == 0``."""
    y = np.asarray(returns, np.float64).reshape(-1)
    pred = np.asarray(values, np.float64).reshape(-1)
    if y.shape != pred.shape or y.size < 1:
        raise ValueError('values and returns must hold the same number (>= 1) of entries')
    var_y = np.var(y)
    return float('nan') if var_y == 0 else float(1.0 - np.var(y - pred) / var_y)


def explained_variance_device(values, returns, out=None, stream=None):
    """``explained_variance_numpy`` as one launch (``ce_explained_variance``):
    ``values`` is a ``[K][rows]`` float32 view of the policy records (every
    record contiguous), ``returns`` the learner's contiguous float32 ``[K][rows]``
    (or flat) tensor.  Returns the float64 device scalar (``out [1]`` or a new
    tensor); nothing is read back."""
    import torch
    from custom_envs_amd import _native
    if values.dim() != 2 or values.dtype != torch.float32 or not values[0].is_contiguous():
        raise ValueError('values must be a float32 [K][rows] view with contiguous records')
    k, rows = (int(v) for v in values.shape)
    if returns.dtype != torch.float32 or returns.numel() != k * rows or not returns.is_contiguous():
        raise ValueError('returns must be a contiguous float32 tensor of K * rows = %d entries'
                         % (k * rows))
    if not values.is_cuda or returns.device != values.device:
        raise ValueError('values and returns must be on one GPU')
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=values.device)
    elif out.dtype != torch.float64 or out.numel() != 1 or out.device != values.device:
        raise ValueError('out must be one float64 on the device of values')
    stride = values.stride(0) * 4 if k > 1 else rows * 4
    if stream is None:
        stream = torch.cuda.current_stream(values.device).cuda_stream
    with torch.cuda.device(values.device):
        _native.check(_native.load().ce_explained_variance(
            k, rows, values.data_ptr(), stride, returns.data_ptr(), out.data_ptr(), stream),
            'ce_explained_variance')
    return out


class DeviceVecMonitor:
    """``VecMonitor`` with the episode bookkeeping on the device: the same
    constructor, surface, rows and ``.mon.csv`` chunks, but the K records of a
    ``collect`` are scanned where the rollout left them (``ce_monitor_scan``:
    ``episodes_numpy`` states it) and only the finished episodes' records come
    to the host.

    ``bind`` (the env calls it) says where the info keywords live in the
    rollout fields.  ``scan(fields, k)`` launches on torch's current stream of
    the device -- the env has waited for the engine by then -- and drains:
    one 8-byte copy of the count and one copy of ``count`` records (a third
    only when the record buffer had to grow, after which the write launch is
    repeated, not the scan).  Rows are stamped ``t`` at the drain.  ``step``
    feeds the same entry a K = 1 record, so mixed ``step`` / ``collect`` use
    keeps one carry.  Per-step ``callbacks`` need the host path and raise
    ``ValueError``.  ``device=None`` builds the argument-checking form, which
    needs no GPU."""
    on_device = True
    KEEP = 100           # finished episodes kept for a learner's ep_info_buf

    def __init__(self, num_envs, file_paths=None, info_keywords=(), chunk_size=1,
                 callbacks=None, style='logging', allow_early_resets=True,
                 reset_keywords=(), device=0):
        from collections import deque
        if style not in ('logging', 'sb'):
            raise ValueError('style must be logging or sb')
        if callbacks:
            raise ValueError('the device monitor takes no callbacks: a per-step Python payload '
                             'needs the host monitor (leave the device switch off)')
        self.style = style
        self.reset_keywords = tuple(reset_keywords or ())
        if self.reset_keywords and style != 'sb':
            raise ValueError('reset_keywords belong to the sb style')
        self.allow_early_resets = bool(allow_early_resets)
        self.num_envs = int(num_envs)
        if self.num_envs < 1:
            raise ValueError('num_envs must be at least 1')
        self.needs_reset = np.ones(self.num_envs, bool)
        if file_paths is None or isinstance(file_paths, (str, Path)):
            file_paths = [file_paths] * self.num_envs if file_paths is None else [
                '%s_%d' % (file_paths, i) for i in range(self.num_envs)]
        if len(file_paths) != self.num_envs:
            raise ValueError('got %d file paths for %d envs' % (len(file_paths), self.num_envs))
        self.paths = [_mon_path(p) for p in file_paths]
        self.info_keywords = tuple(info_keywords)
        from custom_envs_amd._native import CE_MONITOR_MAX_INFO
        if len(self.info_keywords) > CE_MONITOR_MAX_INFO:
            raise ValueError('at most %d info_keywords, got %d'
                             % (CE_MONITOR_MAX_INFO, len(self.info_keywords)))
        self.chunk_size = chunk_size
        self.callbacks = []
        self.t_start = time.time()
        self.data = [[] for _ in range(self.num_envs)]
        self.metric_history = [defaultdict(list) for _ in range(self.num_envs)]
        self.total_steps = np.zeros(self.num_envs, np.int64)
        self.reset_info = [{} for _ in range(self.num_envs)]
        self.device = None if device is None else int(device)
        self.row_stride, self.info_source = 1, None
        self.recent = deque(maxlen=self.KEEP)     # the newest rows, oldest first
        self.n_finished = 0
        self.drained_bytes = 0                    # device-to-host bytes of every drain so far
        self._h = self._lib = self._out = self._total = None
        self._capacity = 0

    # ----------------------------------------------------------------- binding
    def bind(self, info_source, row_stride=1):
        """``info_source``: info keyword -> (rollout field, column); an env's
        reward and done are those of row ``env * row_stride``."""
        missing = [k for k in self.info_keywords if k not in info_source]
        if missing:
            raise ValueError('the device monitor cannot read the info keywords %s from the '
                             'rollout records (it has %s)' % (missing, sorted(info_source)))
        if int(row_stride) < 1:
            raise ValueError('row_stride must be at least 1')
        self.info_source = {k: (str(info_source[k][0]), int(info_source[k][1]))
                            for k in self.info_keywords}
        self.row_stride = int(row_stride)
        return self

    def _handle(self):
        if self._h is None:
            import ctypes
            from custom_envs_amd import _native
            if self.device is None:
                raise RuntimeError('this monitor was built without a device (argument checks only)')
            self._lib = _native.load()
            h = ctypes.c_void_p()
            _native.check(self._lib.ce_monitor_create(self.device, self.num_envs, ctypes.byref(h)),
                          'ce_monitor_create')
            self._h = h
        return self._h

    def _stream(self):
        import torch
        return torch.cuda.current_stream(torch.device('cuda', self.device)).cuda_stream

    # ------------------------------------------------------------- VecMonitor's
    def reset(self, indices=None, **kwargs):
        idx = slice(None) if indices is None else indices
        if self.style == 'sb' and not self.allow_early_resets and not self.needs_reset[idx].all():
            raise RuntimeError('Tried to reset an environment before done. If you want to '
                               'allow early resets, wrap your env with Monitor(env, path, '
                               'allow_early_resets=True)')
        self.needs_reset[idx] = False         # before the keyword check, monitor.py:84-85
        for key in self.reset_keywords:
            if kwargs.get(key) is None:
                raise ValueError('Expected you to pass kwarg %s into reset' % key)
        envs = np.atleast_1d(np.arange(self.num_envs)[idx])
        for i in envs:
            for key in self.reset_keywords:
                self.reset_info[int(i)][key] = kwargs[key]
        from custom_envs_amd._native import check
        h = self._handle()
        if indices is None:
            check(self._lib.ce_monitor_reset(h, None, 0, self._stream()), 'ce_monitor_reset')
        else:
            arr = np.ascontiguousarray(envs, np.int32)
            check(self._lib.ce_monitor_reset(h, arr.ctypes.data, arr.size, self._stream()),
                  'ce_monitor_reset')

    def check_step(self):
        if self.style == 'sb' and self.needs_reset.any():
            raise RuntimeError('Tried to step environment that needs reset')

    def get_state(self):
        """The carry as ``new_carry``'s dict (synchronises)."""
        from custom_envs_amd._native import check
        c = new_carry(self.num_envs)
        check(self._lib.ce_monitor_get_state(
            self._handle(), c['ep_reward'].ctypes.data, c['ep_len'].ctypes.data,
            c['episode'].ctypes.data, c['total_steps'].ctypes.data, self._stream()),
            'ce_monitor_get_state')
        return c

    def set_state(self, carry):
        from custom_envs_amd._native import check
        ref = new_carry(self.num_envs)
        c = {}
        for name, like in ref.items():
            v = np.ascontiguousarray(carry[name], like.dtype)
            if v.shape != like.shape:
                raise ValueError('carry %s must have shape %s, got %s' % (name, like.shape, v.shape))
            c[name] = v
        check(self._lib.ce_monitor_set_state(
            self._handle(), c['ep_reward'].ctypes.data, c['ep_len'].ctypes.data,
            c['episode'].ctypes.data, c['total_steps'].ctypes.data, self._stream()),
            'ce_monitor_set_state')
        self.total_steps[:] = c['total_steps']

    # -------------------------------------------------------------------- scan
    def _columns(self, fields, k, source):
        import torch
        from custom_envs_amd._native import CeMonitorColumn
        cols = (CeMonitorColumn * max(1, len(self.info_keywords)))()
        for j, key in enumerate(self.info_keywords):
            name, col = source[key]
            t = fields.get(name)
            if t is None:
                raise ValueError('the rollout fields lack %r (info keyword %r)' % (name, key))
            self._check_field(name, t, torch.float32, k)
            row_floats = t[0].numel() // self.num_envs
            if t[0].numel() != row_floats * self.num_envs or not 0 <= col < row_floats:
                raise ValueError('%s holds %d floats per record: no column %d for %d envs'
                                 % (name, t[0].numel(), col, self.num_envs))
            cols[j] = CeMonitorColumn(t.data_ptr(), self._stride(t, k), row_floats, col)
        return cols

    def _check_field(self, name, t, dtype, k):
        if not hasattr(t, 'data_ptr') or t.dtype != dtype:
            raise ValueError('%s must be a %s tensor, got %s'
                             % (name, dtype, getattr(t, 'dtype', type(t).__name__)))
        if t.dim() < 2 or t.shape[0] < k or not t[0].is_contiguous():
            raise ValueError('%s must hold at least %d contiguous records, got shape %s'
                             % (name, k, tuple(t.shape)))
        if not t.is_cuda or t.device.index != self.device:
            raise ValueError('%s must be on cuda:%d, got %s' % (name, self.device, t.device))

    @staticmethod
    def _stride(t, k):
        return t.stride(0) * t.element_size() if t.shape[0] > 1 else t[0].numel() * t.element_size()

    def _reserve(self, capacity, record_bytes):
        import torch
        if self._out is None or self._out.numel() < capacity * record_bytes:
            self._out = torch.empty(capacity * record_bytes, dtype=torch.uint8,
                                    device=torch.device('cuda', self.device))
        self._capacity = self._out.numel() // record_bytes

    def scan(self, fields, k, row_stride=None, source=None):
        """``k`` records of ``fields`` (``reward`` float32 and ``done`` uint8
        ``[>= k][rows]`` device views, and the fields ``bind`` named) through
        the monitor; returns the finished episodes' rows, in (t, env) order, as
        ``(env, ep_info)`` pairs."""
        import torch
        from custom_envs_amd._native import check
        k = int(k)
        if k < 1:
            raise ValueError('k must be at least 1, got %d' % k)
        source = self.info_source if source is None else source
        if self.info_keywords and source is None:
            raise RuntimeError('bind() the monitor to its env\'s rollout fields first')
        row_stride = self.row_stride if row_stride is None else int(row_stride)
        h = self._handle()
        reward, done = fields['reward'], fields['done']
        self._check_field('reward', reward, torch.float32, k)
        self._check_field('done', done, torch.uint8, k)
        rows = self.num_envs * row_stride
        if reward[0].numel() < rows or done[0].numel() < rows:
            raise ValueError('reward / done records hold fewer than %d rows' % rows)
        cols = self._columns(fields, k, source)
        n_info = len(self.info_keywords)
        dtype = record_dtype(n_info)
        rb = dtype.itemsize
        if self._total is None:
            self._total = torch.zeros(1, dtype=torch.int64, device=torch.device('cuda', self.device))
        self._reserve(max(self._capacity, 1024, 2 * self.num_envs), rb)
        stream = self._stream()
        check(self._lib.ce_monitor_scan(
            h, k, self.num_envs, row_stride, reward.data_ptr(), self._stride(reward, k),
            done.data_ptr(), self._stride(done, k), cols, n_info, self._out.data_ptr(),
            self._capacity, self._total.data_ptr(), stream), 'ce_monitor_scan')
        self.total_steps += k
        total = int(self._total.item())                    # copy 1: the count
        self.drained_bytes += 8
        if total > self._capacity:                         # grow, repeat the write alone
            cap = 1 << (total - 1).bit_length()
            self._out = None
            self._reserve(cap, rb)
            check(self._lib.ce_monitor_write(h, self._out.data_ptr(), self._capacity, stream),
                  'ce_monitor_write')
        if total == 0:
            return []
        host = self._out[:total * rb].cpu().numpy().view(dtype)      # copy 2: the records
        self.drained_bytes += total * rb
        return self._append(host)

    def _append(self, records):
        """The rows of ``records`` into ``data``, ``metric_history`` and the
        files, as ``VecMonitor.step`` appends them."""
        now = time.time() - self.t_start
        t_row = round(now, 6)
        if self.reset_keywords and len(records):
            # the host monitor's auto-reset raises after the first step with a done
            records = records[records['t'] == records['t'][0]]
        # the fields as Python lists, converted once (float32 -> float exactly)
        envs, rs, ls = records['env'].tolist(), records['r'].tolist(), records['l'].tolist()
        logging = self.style == 'logging'
        currents = records['current_reward'].astype(np.float64).tolist() if logging else None
        episodes = records['episode'].tolist() if logging else None
        keys = self.info_keywords
        infos = records['info'].astype(np.float64).tolist() if keys else None
        data, paths, chunk, histories = self.data, self.paths, self.chunk_size, self.metric_history
        out = []
        for n, i in enumerate(envs):
            r, l = rs[n], ls[n]
            ep_info = {'r': round(r, 6), 'l': l, 't': t_row}
            if logging:
                ep_info['current_reward'] = currents[n]
                ep_info['episode'] = episodes[n]
            if keys:
                ep_info.update(zip(keys, infos[n]))
            if self.reset_info[i]:
                ep_info.update(self.reset_info[i])
            rows = data[i]
            rows.append(ep_info)
            if len(rows) >= chunk:
                _save_rows(paths[i], rows)
                data[i] = []
            history = histories[i]
            history['rewards'].append(r)
            history['lengths'].append(l)
            history['times'].append(now)
            out.append((i, ep_info))
        self.recent.extend(ep_info for _, ep_info in out[-self.KEEP:])
        self.n_finished += len(out)
        if out and self.reset_keywords:      # the auto-reset passes no kwargs (VecMonitor.step)
            raise ValueError('Expected you to pass kwarg %s into reset' % self.reset_keywords[0])
        return out

    def step(self, rewards, dones, infos, observations=None, fields=None):
        """``VecMonitor.step`` for one step's host arrays (``rewards``: the
        engine's float32 values): the same scan entry with a K = 1 record.
        ``fields``: the step's host output arrays by rollout field name, read
        as ``bind`` says; without them the info keywords are taken from
        ``infos[i][key]``.  Returns {env: ep_info} of the envs that finished."""
        import torch
        E = self.num_envs
        dev = torch.device('cuda', self.device)
        n_info = len(self.info_keywords)
        info = np.zeros((1, E, max(1, n_info)), np.float32)
        for j, key in enumerate(self.info_keywords):
            if fields is not None:
                name, col = self.info_source[key]
                info[0, :, j] = np.asarray(fields[name], np.float32).reshape(E, -1)[:, col]
            else:
                info[0, :, j] = [infos[i][key] for i in range(E)]
        rec = {'reward': torch.from_numpy(np.ascontiguousarray(
                   np.asarray(rewards, np.float32).reshape(1, E))).to(dev),
               'done': torch.from_numpy(np.ascontiguousarray(
                   (np.asarray(dones) != 0).astype(np.uint8).reshape(1, E))).to(dev),
               '_info': torch.from_numpy(info).to(dev)}
        source = {key: ('_info', j) for j, key in enumerate(self.info_keywords)}
        return dict(self.scan(rec, 1, row_stride=1, source=source))

    def close(self):
        for i in range(self.num_envs):
            _save_rows(self.paths[i], self.data[i])
            self.data[i] = []
        if self._h is not None:
            self._lib.ce_monitor_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            if self._h is not None:
                self._lib.ce_monitor_destroy(self._h)
                self._h = None
        except Exception:
            pass

    get_episode_rewards = VecMonitor.get_episode_rewards
    get_episode_lengths = VecMonitor.get_episode_lengths
    get_episode_times = VecMonitor.get_episode_times
    get_total_steps = VecMonitor.get_total_steps


def make_vec_monitor(num_envs, paths, mkw, device=0):
    """The monitor a vec env attaches for ``(paths, mkw)``: ``VecMonitor``, or
    with ``mkw['device']`` true the ``DeviceVecMonitor`` on ``device``."""
    kwargs = dict(info_keywords=mkw.get('info_keywords', ()), chunk_size=mkw.get('chunk_size', 1),
                  callbacks=mkw.get('callbacks'), style=mkw.get('style', 'logging'),
                  allow_early_resets=mkw.get('allow_early_resets', True),
                  reset_keywords=mkw.get('reset_keywords', ()))
    if mkw.get('device'):
        return DeviceVecMonitor(num_envs, paths, device=device, **kwargs)
    return VecMonitor(num_envs, paths, **kwargs)


def create_env(env_name, log_dir=None, num_of_envs=1, **kwargs):
    """utils_logging.py:159-175."""
    from custom_envs_amd.core import make
    envs = [make(env_name, **kwargs) for _ in range(num_of_envs)]
    if log_dir is not None:
        log_dir = Path(log_dir)
        envs = [Monitor(env, str(log_dir / str(i)), chunk_size=10,
                        info_keywords=('objective', 'accuracy'))
                for i, env in enumerate(envs)]
    return envs
