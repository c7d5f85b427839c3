"""The agent's policy on the device: stable-baselines' ``MlpPolicy`` as one
fused HIP launch (``ce_policy_*``, csrc/policy_kernels.h).

PPO2 / A2C pick step t+1's action from step t's observation
(run_multiagent_exp_single.py:37-49).  ``MlpPolicy`` holds that network in the
engine -- two separate tanh MLPs (``net_arch=[dict(pi=hidden, vf=hidden)]``),
a linear mean head, a linear value head, a state-independent ``logstd`` -- so
``OptimizeEngine.rollout_policy`` / ``MultiOptEngine.rollout_policy`` can
enqueue ``[policy, env step] x K`` with no host work between steps.

Semantics (``forward_numpy`` is their executable statement):

    mean       = tanh-MLP_pi(obs) @ Wmu + bmu
    value      = tanh-MLP_vf(obs) @ Wv + bv
    action     = mean + exp(logstd) * noise        (noise None: action = mean)
    env_action = clip(action, low, high)           (what the env reads; action
                                                    stays unclipped, as SB's
                                                    runner stores it)
    neglogp    = 0.5 sum(noise^2) + sum(logstd) + 0.5 A log(2 pi)

``neglogp`` is computed from the noise itself, not from ``(action - mean) /
std``: the two agree in exact arithmetic, and the noise form does not lose
digits when ``std`` is small.  The noise is an input: a tensor (``collect`` draws one
``torch.randn`` per rollout by default), or a ``custom_envs_amd.rng.DeviceRng``,
with which the kernel forms its noise itself from the counter-based generator
(csrc/rng.h) -- bit-equal to feeding it ``rng.normal(...)``, with no noise
tensor written or read.

Limits: 1-3 hidden layers, each width a multiple of 32 up to 128, obs_dim <=
128, act_dim <= 64.  Anything else raises ``NativeEngineError``
(CE_EUNSUPPORTED); there is no eager fallback.  The reference's default
7x7-image Optimize shape (981 wide, 490 actions) takes ``WideMlpPolicy``
(obs_dim <= 1024, act_dim <= 512; csrc/policy_wide_kernels.h): the act side --
forwards, rollouts, ``collect``, ``VecNormalize`` -- with the same interface;
the learners refuse it.
"""
import ctypes
from collections import OrderedDict

import numpy as np

from custom_envs_amd import _native
from custom_envs_amd._native import CePolicyConfig, CePolicyOutputs, check

POLICY_FIELDS = ('action', 'env_action', 'neglogp', 'value')
LOG_2PI = float(np.log(2.0 * np.pi))


def params_layout(obs_dim, act_dim, hidden):
    """Ordered name -> (offset, shape) of the flat float32 parameter vector:
    the pi network ``pi/w0, pi/b0, ..., pi/w_out [h][A], pi/b_out``, the vf
    network ``vf/w0, ..., vf/w_out [h][1], vf/b_out``, then ``logstd [A]``.
    Kernels are row-major ``[in][out]``."""
    layout, off = OrderedDict(), 0

    def add(name, shape):
        nonlocal off
        layout[name] = (off, tuple(shape))
        off += int(np.prod(shape))

    for net, out in (('pi', act_dim), ('vf', 1)):
        width = obs_dim
        for i, h in enumerate(hidden):
            add('%s/w%d' % (net, i), (width, h))
            add('%s/b%d' % (net, i), (h,))
            width = h
        add('%s/w_out' % net, (width, out))
        add('%s/b_out' % net, (out,))
    add('logstd', (act_dim,))
    return layout


def layout_size(layout):
    off, shape = next(reversed(layout.values()))
    return off + int(np.prod(shape))


def flat_to_dict(flat, layout):
    flat = np.asarray(flat).reshape(-1)
    if flat.size != layout_size(layout):
        raise ValueError('flat parameter vector has %d entries, the layout %d'
                         % (flat.size, layout_size(layout)))
    return OrderedDict((name, flat[off:off + int(np.prod(shape))].reshape(shape))
                       for name, (off, shape) in layout.items())


def dict_to_flat(params, layout, dtype=np.float32):
    if set(params) != set(layout):
        raise ValueError('parameter names differ from the layout: %s'
                         % sorted(set(params) ^ set(layout)))
    flat = np.empty(layout_size(layout), dtype)
    for name, (off, shape) in layout.items():
        value = np.asarray(params[name])
        if value.shape != shape:
            raise ValueError('%s has shape %s, the layout %s' % (name, value.shape, shape))
        flat[off:off + value.size] = value.reshape(-1)
    return flat


def forward_numpy(obs, noise=None, params=None, hidden=(64, 64), low=None, high=None,
                  dtype=np.float64):
    """The policy in plain NumPy, in ``dtype``: the checker of the kernel and
    the statement of its semantics.  ``params``: the flat vector or the dict
    of ``params_layout``.  Returns a dict of ``action``, ``env_action``
    ``[rows][A]``, ``neglogp``, ``value`` ``[rows]`` and ``mean``.  ``neglogp``
    comes from the noise itself (0.5 sum noise^2 + sum logstd + 0.5 A log 2 pi,
    sum noise^2 = 0 without noise), not from (action - mean) / std."""
    obs = np.asarray(obs, dtype)
    if not isinstance(params, dict):
        flat = np.asarray(params).reshape(-1)
        # A from the vector's length: n = fixed(D, hidden) + A (h_last + 2) + ...
        D, width, fixed = obs.shape[1], obs.shape[1], 0
        for h in hidden:
            fixed += 2 * (width * h + h)
            width = h
        fixed += width + 1
        n_act = (flat.size - fixed) // (width + 2)
        params = flat_to_dict(flat, params_layout(D, n_act, hidden))
    p = {k: np.asarray(v, dtype) for k, v in params.items()}

    def mlp(net):
        x = obs
        for i in range(len(hidden)):
            x = np.tanh(x @ p['%s/w%d' % (net, i)] + p['%s/b%d' % (net, i)])
        return x @ p['%s/w_out' % net] + p['%s/b_out' % net]

    mean = mlp('pi')
    value = mlp('vf')[:, 0]
    logstd = p['logstd']
    n_act = logstd.size
    if noise is None:
        action, sq = mean.copy(), np.zeros(obs.shape[0], dtype)
    else:
        noise = np.asarray(noise, dtype)
        action = mean + np.exp(logstd) * noise
        sq = np.sum(noise * noise, axis=1)
    lo = -np.inf if low is None else np.asarray(low, dtype)
    hi = np.inf if high is None else np.asarray(high, dtype)
    neglogp = (0.5 * sq + np.sum(logstd) + 0.5 * n_act * LOG_2PI).astype(dtype)
    return {'action': action, 'env_action': np.minimum(np.maximum(action, lo), hi),
            'neglogp': neglogp, 'value': value, 'mean': mean}


def _bounds(value, act_dim):
    if value is None:
        return None
    return np.ascontiguousarray(np.broadcast_to(np.asarray(value, np.float32), (act_dim,)))


class MlpPolicy:
    """The actor-critic MLP on one GPU (see the module docstring).
    ``device=None`` builds the shape only -- ``params_layout``,
    ``forward_numpy`` and the argument checks, which need no GPU."""
    # the two C functions a policy is created through
    N_PARAMS_FN = 'ce_policy_n_params'
    CREATE_FN = 'ce_policy_create'

    def __init__(self, obs_dim, act_dim, hidden=(64, 64), low=None, high=None, device=0):
        lib = _native.load()
        self.obs_dim, self.act_dim = int(obs_dim), int(act_dim)
        self.hidden = tuple(int(h) for h in hidden)
        self.device = 0 if device is None else int(device)
        if len(self.hidden) > 4:
            raise _native.NativeEngineError('the policy takes 1 to 3 hidden layers')
        self._cfg = cfg = CePolicyConfig(abi_version=_native.ABI_VERSION, device=self.device,
                                         obs_dim=self.obs_dim, act_dim=self.act_dim,
                                         n_hidden=len(self.hidden))
        for i, h in enumerate(self.hidden):
            cfg.hidden[i] = h
        n = getattr(lib, self.N_PARAMS_FN)(ctypes.byref(cfg))
        if n < 0:
            check(n, self.N_PARAMS_FN)
        self.n_params = int(n)
        self._lib, self._h = lib, None
        self.low, self.high = _bounds(low, self.act_dim), _bounds(high, self.act_dim)
        if device is None:      # shape only: layout, forward_numpy and validation, no GPU
            return
        handle = ctypes.c_void_p()
        check(getattr(lib, self.CREATE_FN)(ctypes.byref(cfg), ctypes.byref(handle)), self.CREATE_FN)
        self._h = handle
        if low is not None or high is not None:
            check(lib.ce_policy_set_bounds(
                handle, None if self.low is None else self.low.ctypes.data,
                None if self.high is None else self.high.ctypes.data), 'ce_policy_set_bounds')

    def params_layout(self):
        return params_layout(self.obs_dim, self.act_dim, self.hidden)

    @staticmethod
    def _stream(stream):
        if stream is not None:
            return ctypes.c_void_p(stream or 0)
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream or 0)

    def set_params(self, params, stream=None):
        """``params``: the flat vector or the ``params_layout`` dict, as numpy
        (copied and synchronised) or a float32 torch tensor on this device
        (one repacking launch on ``stream`` -- default: torch's current
        stream -- with no host round trip)."""
        if isinstance(params, dict):
            params = dict_to_flat(params, self.params_layout())
        if isinstance(params, np.ndarray) or not hasattr(params, 'data_ptr'):
            flat = np.ascontiguousarray(params, dtype=np.float32).reshape(-1)
            if flat.size != self.n_params:
                raise ValueError('got %d parameters, the policy has %d' % (flat.size, self.n_params))
            check(self._lib.ce_policy_set_params(self._h, flat.ctypes.data, flat.size, 0,
                                                 self._stream(stream)), 'ce_policy_set_params')
            self._host_params = flat.copy()
            return
        import torch
        if (params.dtype != torch.float32 or not params.is_contiguous()
                or params.device.type != 'cuda' or params.device.index != self.device):
            raise ValueError('device parameters must be a contiguous float32 tensor on cuda:%d'
                             % self.device)
        if params.numel() != self.n_params:
            raise ValueError('got %d parameters, the policy has %d' % (params.numel(), self.n_params))
        check(self._lib.ce_policy_set_params(self._h, params.data_ptr(), params.numel(),
                                             _native.CE_PTR_DEVICE, self._stream(stream)),
              'ce_policy_set_params')
        self._host_params = None

    # ------------------------------------------------------------- validation
    def check_outputs(self, out, rows, k=None, record_bytes=None, placement=True):
        """Validate the policy output tensors of one forward (``k`` None: each
        ``(rows, ...)``) or of a K-step rollout (each ``(>= k, rows, ...)``
        with record stride ``record_bytes``) before a pointer reaches C."""
        import torch
        for name in POLICY_FIELDS:
            v = out.get(name)
            if v is None:
                raise ValueError('policy outputs lack %r' % name)
            tail = (rows, self.act_dim) if name in ('action', 'env_action') else (rows,)
            if v.dtype != torch.float32:
                raise ValueError('policy output %s must have dtype float32, got %s' % (name, v.dtype))
            if k is None:
                if tuple(v.shape) != tail:
                    raise ValueError('policy output %s must have shape %s, got %s'
                                     % (name, tail, tuple(v.shape)))
                if not v.is_contiguous():
                    raise ValueError('policy output %s must be contiguous' % name)
                self.check_device('policy output ' + name, v)
                continue
            if tuple(v.shape[1:]) != tail:
                raise ValueError('policy output %s records have shape %s, the policy writes %s'
                                 % (name, tuple(v.shape[1:]), tail))
            if v.shape[0] < k:
                raise ValueError('policy output %s holds %d records, the call writes %d'
                                 % (name, v.shape[0], k))
            if k > 1 and v.stride(0) * v.element_size() != int(record_bytes):
                raise ValueError('policy record_bytes %d is not output %s\'s record stride (%d B)'
                                 % (record_bytes, name, v.stride(0) * v.element_size()))
            if not v[0].is_contiguous():
                raise ValueError('policy output %s: every record must be contiguous' % name)
            if placement:
                self.check_placement('policy output ' + name, v)

    def check_input(self, name, t, shape, placement=True):
        """dtype, shape, contiguity, then the device (in that order, so each
        fault is named even for a tensor that is not on the GPU)."""
        import torch
        if t.dtype != torch.float32:
            raise ValueError('%s must have dtype float32, got %s' % (name, t.dtype))
        if tuple(t.shape) != tuple(shape):
            raise ValueError('%s must have shape %s, got %s' % (name, tuple(shape), tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError('%s must be contiguous' % name)
        if placement:
            self.check_device(name, t)

    def check_device(self, name, t):
        if t.device.type != 'cuda' or t.device.index != self.device:
            raise ValueError('%s must be on device cuda:%d, got %s' % (name, self.device, t.device))

    def check_placement(self, name, t):
        """On this policy's device and 16-byte aligned."""
        self.check_device(name, t)
        if t.data_ptr() % 16:
            raise ValueError('%s must be 16-byte aligned' % name)

    def alloc_outputs(self, rows, k=None):
        """The four output tensors of one forward, or of k rollout records
        (fields of shape ``(k, rows, ...)``; returns ``(fields, record_bytes)``:
        one buffer, 256-byte aligned segments per record)."""
        import torch
        dev = torch.device('cuda', self.device)
        shapes = {n: (rows, self.act_dim) if n in ('action', 'env_action') else (rows,)
                  for n in POLICY_FIELDS}
        if k is None:
            return {n: torch.empty(s, dtype=torch.float32, device=dev) for n, s in shapes.items()}
        offs, rec = {}, 0
        for n, s in shapes.items():
            offs[n] = rec
            rec += -(-int(np.prod(s)) * 4 // 256) * 256
        buf = torch.zeros(int(k) * rec // 4, dtype=torch.float32, device=dev)
        fields = {}
        for n, s in shapes.items():
            strides = (rec // 4, s[1], 1) if len(s) == 2 else (rec // 4, 1)
            fields[n] = buf.as_strided((int(k),) + s, strides, offs[n] // 4)
        fields['_buffer'] = buf
        return fields, rec

    @staticmethod
    def outputs_struct(out):
        return CePolicyOutputs(**{n: out[n].data_ptr() for n in POLICY_FIELDS})

    def forward_device(self, obs, noise=None, out=None, stream=None):
        """One stream-ordered launch over ``obs [rows][D]`` (any engine's obs
        tensor; ``noise [rows][A]``, None, or a ``DeviceRng``, whose draw
        ``t`` the kernel forms itself, without advancing it) on ``stream``
        (default: torch's current stream).  Returns ``out`` (allocated when
        None): ``action``, ``env_action``, ``neglogp``, ``value``."""
        from custom_envs_amd.rng import DeviceRng
        rows = int(obs.shape[0]) if obs.dim() == 2 else -1
        self.check_input('obs', obs, (max(rows, 1), self.obs_dim))
        generated = isinstance(noise, DeviceRng)
        if generated:
            check_rng(noise, self.device, 1, rows)
        elif noise is not None:
            self.check_input('noise', noise, (rows, self.act_dim))
        if out is None:
            out = self.alloc_outputs(rows)
        self.check_outputs(out, rows)
        o = self.outputs_struct(out)
        if generated:
            check(self._lib.ce_policy_forward_rng(self._h, obs.data_ptr(), noise.seed, int(noise.t),
                                                  noise.row_offset, rows, ctypes.byref(o),
                                                  self._stream(stream)), 'ce_policy_forward_rng')
            return out
        check(self._lib.ce_policy_forward(self._h, obs.data_ptr(),
                                          None if noise is None else noise.data_ptr(), rows,
                                          ctypes.byref(o), self._stream(stream)), 'ce_policy_forward')
        return out

    def forward_numpy(self, obs, noise=None, params=None, dtype=np.float64):
        """``forward_numpy`` of this policy's shape and bounds (no GPU)."""
        if params is None:
            params = getattr(self, '_host_params', None)
        if params is None:
            raise ValueError('forward_numpy needs the parameters: none were set from the host '
                             '(the device copy is not read back)')
        return forward_numpy(obs, noise, params, self.hidden, self.low, self.high, dtype)

    def close(self):
        if getattr(self, '_h', None):
            self._lib.ce_policy_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WideMlpPolicy(MlpPolicy):
    """``MlpPolicy`` for obs_dim <= 1024 and act_dim <= 512 (hidden layers as
    there): the reference's default ``Optimize-v0`` shape, 981 -> 490.  The
    same interface, parameter vector and semantics, run by the wide kernel
    (csrc/policy_wide_kernels.h), which at a shape ``MlpPolicy`` takes too
    writes the same bits.  Act side only: ``PPO2Learner`` / ``A2CLearner``
    raise ``NativeEngineError`` for it."""
    N_PARAMS_FN = 'ce_policy_wide_n_params'
    CREATE_FN = 'ce_policy_create_wide'


def check_rng(rng, device, k, rows):
    """A ``DeviceRng`` given as a call's noise: it lives on ``device``, and
    draws ``t .. t + k - 1`` and rows ``row_offset .. row_offset + rows - 1``
    fit 32 bits."""
    if rng.device != device:
        raise ValueError('the generator lives on %s, the policy on cuda:%d'
                         % ('no device' if rng.device is None else 'cuda:%d' % rng.device, device))
    rng.check_draws(k)
    if rng.row_offset + max(int(rows), 0) > 2 ** 32:
        raise ValueError('rows row_offset .. row_offset + rows - 1 must stay below 2^32')


def check_env_records(spec, num_envs, k, fields, record_bytes):
    """The form of the env records of a ``rollout_policy`` call (``spec``: the
    engine's ``output_fields()``): every field a ``(>= k, rows, ...)`` view of
    the engine's dtype whose record stride is ``record_bytes``, each record
    contiguous.  Returns the first record's tensors."""
    for name, dtype, rows, tail in spec:
        v = fields.get(name)
        if v is None:
            raise ValueError('rollout fields lack %r' % name)
        if v.dtype != dtype:
            raise ValueError('field %s must have dtype %s, got %s' % (name, dtype, v.dtype))
        if tuple(v.shape[1:]) != (num_envs * rows,) + tuple(tail):
            raise ValueError('field %s records have shape %s, the engine writes %s'
                             % (name, tuple(v.shape[1:]), (num_envs * rows,) + tuple(tail)))
        if v.shape[0] < k:
            raise ValueError('field %s holds %d records, the call writes %d' % (name, v.shape[0], k))
        if k > 1 and v.stride(0) * v.element_size() != int(record_bytes):
            raise ValueError('record_bytes %d is not field %s\'s record stride (%d B)'
                             % (record_bytes, name, v.stride(0) * v.element_size()))
        if int(record_bytes) % 16:
            raise ValueError('record_bytes must be a multiple of 16, got %d' % record_bytes)
        if not v[0].is_contiguous():
            raise ValueError('field %s: every record must be contiguous' % name)
    return {n: v[0] for n, v in fields.items() if n != '_buffer'}


def validate_rollout(spec, num_envs, rows, obs_dim, act_dim, device, k, policy, obs0, noise,
                     fields, record_bytes, policy_fields, policy_record_bytes=None):
    """Every check of ``rollout_policy`` (both engines call this before a
    pointer reaches C; it needs no engine, so it runs without a GPU up to the
    device checks, which come last).  ``noise``: a ``[>= k][rows][A]``
    tensor, None, or a ``DeviceRng``.  Returns (first env record, policy
    record bytes)."""
    from custom_envs_amd.rng import DeviceRng
    generated = isinstance(noise, DeviceRng)
    if generated:
        rng, noise = noise, None
    if not isinstance(policy, MlpPolicy):
        raise TypeError('policy must be an MlpPolicy')
    if (policy.obs_dim, policy.act_dim) != (obs_dim, act_dim):
        raise ValueError('the policy maps obs_dim %d -> act_dim %d, the engine\'s rows are %d -> %d'
                         % (policy.obs_dim, policy.act_dim, obs_dim, act_dim))
    if policy.device != device:
        raise ValueError('the policy lives on cuda:%d, the engine on cuda:%d'
                         % (policy.device, device))
    k = int(k)
    if k < 1:
        raise ValueError('k must be >= 1, got %d' % k)
    if policy_record_bytes is None:
        first = policy_fields.get('action')
        if first is None:
            raise ValueError("policy outputs lack 'action'")
        policy_record_bytes = first.stride(0) * first.element_size()
    if int(policy_record_bytes) % 16:
        raise ValueError('policy record_bytes must be a multiple of 16, got %d' % policy_record_bytes)
    if noise is not None and (noise.dim() != 3 or noise.shape[0] < k):
        raise ValueError('noise must be [>= k][rows][A]; got shape %s for k = %d'
                         % (tuple(noise.shape), k))
    # the form of every tensor first, then where it lives
    first = check_env_records(spec, num_envs, k, fields, record_bytes)
    policy.check_outputs(policy_fields, rows, k, policy_record_bytes, placement=False)
    policy.check_input('obs0', obs0, (rows, obs_dim), placement=False)
    if noise is not None:
        policy.check_input('noise', noise, (noise.shape[0], rows, act_dim), placement=False)
        policy.check_device('noise', noise)
    if generated:
        check_rng(rng, device, k, rows)
    policy.check_placement('obs0', obs0)
    for name, _, _, _ in spec:
        policy.check_placement('field ' + name, fields[name])
    for name in POLICY_FIELDS:
        policy.check_placement('policy output ' + name, policy_fields[name])
    return first, int(policy_record_bytes)
