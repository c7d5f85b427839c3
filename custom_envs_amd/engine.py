"""Python handle on one HIP Optimize-v0 engine (one GPU, E envs).

``OptimizeEngine`` is the thin host layer over the C ABI: it builds the
config, seeds envs with gym semantics, and moves actions/outputs either
through the engine's pinned host buffers (numpy in, numpy out) or straight
between device tensors (``step_device``; torch tensors on the engine
stream, no host round trip).  There is no CPU fallback: constructing an
engine without the HIP library or without a GPU raises
``NativeEngineError``.
"""
import ctypes
import os

import numpy as np

from custom_envs_amd import _native
from custom_envs_amd._native import CeConfig, CeOutputs, CeState, check

PRECISIONS = {'f64': _native.CE_F64, 'float64': _native.CE_F64,
              'f32': _native.CE_F32, 'float32': _native.CE_F32}
MODELS = {'linear': _native.CE_PROBLEM_SOFTMAX, 'mlp': _native.CE_PROBLEM_MLP}


def normalize_seed(seed):
    """gym ``create_seed``: None -> 64 random bits, int -> int mod 2**64."""
    if seed is None:
        return int.from_bytes(os.urandom(8), 'little')
    if isinstance(seed, (int, np.integer)) and seed >= 0:
        return int(seed) % (1 << 64)
    raise ValueError('seed must be a non-negative integer or None, got %r' % (seed,))


def labels_from_targets(targets):
    """Class index per row of one-hot targets (argmax(Y), optimize.py:94-96)."""
    targets = np.asarray(targets)
    if targets.ndim == 1:
        return targets.astype(np.int32), int(targets.max()) + 1
    return np.argmax(targets, axis=1).astype(np.int32), targets.shape[1]


def _view(ptr, count, ctype, dtype, shape):
    buf = (ctype * count).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype).reshape(shape)


def compact_derived(n_params, max_steps):
    """The full obs rows, the done flags and the reward from the compact
    fields.  reward = -loss and objective = loss in the reference when B = N
    (optimize.py:91,94-97: the full-data pass IS the minibatch), and
    float32(-x) = -float32(x), so -objective is the reward bit for bit."""
    import torch

    def obs(f):
        tail = f['obs_tail']
        full = torch.zeros((tail.shape[0], 2 * n_params + 1), dtype=tail.dtype, device=tail.device)
        full[:, n_params:] = tail
        return full

    def done(f):
        return (f['episode_len'] >= max_steps).to(torch.uint8)

    def reward(f):
        return -f['objective']

    return {'obs': obs, 'done': done, 'reward': reward}


def check_rollout(spec, num_envs, k, actions, act_count, fields, record_bytes,
                  per_step_actions=True):
    """Validate a K-step strided call before its pointers reach the kernel
    (``ce_step_many_strided`` / ``ce_multi_step_many_strided`` write record t
    at ``t * record_bytes`` for t < k and read k action blocks).

    ``spec``: the engine's ``output_fields()``.  Every field must be a
    (>= k, rows, ...) view of the engine's dtype whose record stride IS
    ``record_bytes``, each record contiguous and 16-byte aligned; the actions
    a contiguous float32 device tensor of at least k (or 1) blocks."""
    import torch
    k = int(k)
    if k < 1:
        raise ValueError('k must be >= 1, got %d' % k)
    if (actions.dtype != torch.float32 or not actions.is_contiguous()
            or actions.device.type != 'cuda'):
        raise ValueError('actions must be a contiguous float32 device tensor')
    if actions.numel() < (k if per_step_actions else 1) * act_count:
        raise ValueError('actions tensor too small: %d floats for %d steps of %d'
                         % (actions.numel(), k if per_step_actions else 1, act_count))
    for name, dtype, rows, tail in spec:
        v = fields.get(name)
        if v is None:
            raise ValueError('rollout fields lack %r' % name)
        if v.dtype != dtype or v.device.type != 'cuda':
            raise ValueError('field %s must be a %s device tensor' % (name, dtype))
        if tuple(v.shape[1:]) != (num_envs * rows,) + tuple(tail):
            raise ValueError('field %s records have shape %s, the engine writes %s'
                             % (name, tuple(v.shape[1:]), (num_envs * rows,) + tuple(tail)))
        if v.shape[0] < k:
            raise ValueError('field %s holds %d records, the call writes %d' % (name, v.shape[0], k))
        if k > 1 and v.stride(0) * v.element_size() != int(record_bytes):
            raise ValueError('record_bytes %d is not field %s\'s record stride (%d B)'
                             % (record_bytes, name, v.stride(0) * v.element_size()))
        if not v[0].is_contiguous() or v.data_ptr() % 16:
            raise ValueError('field %s: every record must be contiguous and 16-byte aligned' % name)
    return {n: v[0] for n, v in fields.items() if n != '_buffer'}


def make_config(n_rows, n_features, n_classes, num_envs, batch_size=None, max_steps=40,
                precision=None, device=0, auto_reset=True, model='linear', hidden=64):
    """The ``ce_config`` of an ``OptimizeEngine`` with these arguments (the
    engine plans its kernel path from it and the CE_* environment switches)."""
    if model not in MODELS:
        raise ValueError('model must be one of %s' % sorted(MODELS))
    if precision is None:
        precision = 'f32' if model == 'mlp' else 'f64'
    layers = (int(hidden),) if np.isscalar(hidden) else tuple(int(h) for h in hidden)
    if model == 'mlp' and not 1 <= len(layers) <= 4:
        raise ValueError('hidden: 1 to 4 layer widths')
    cfg = CeConfig(abi_version=_native.ABI_VERSION, problem=MODELS[model],
                   precision=PRECISIONS[precision], device=int(device),
                   num_envs=int(num_envs), n_rows=n_rows, n_features=n_features,
                   n_classes=n_classes, batch_size=n_rows if batch_size is None else int(batch_size),
                   max_steps=int(max_steps), auto_reset=1 if auto_reset else 0,
                   n_hidden=layers[0] if model == 'mlp' else 0,
                   n_layers=len(layers) if model == 'mlp' and len(layers) > 1 else 0)
    for i, width in enumerate(layers if model == 'mlp' else ()):
        cfg.hidden[i] = width
    return cfg


class OptimizeEngine:
    """E Optimize-v0 environments advanced in lock step on one GPU."""

    def __init__(self, features, targets, num_envs, batch_size=None, max_steps=40,
                 precision=None, device=0, auto_reset=True, model='linear', hidden=64):
        """``model``: 'linear' (the build-defined ModelNumpy softmax classifier,
        float64 by default) or 'mlp' (the OptimizeNN network: F -> hidden...
        relu -> K softmax, float32; ``hidden`` a width or up to 4
        widths; hidden=64 with batch_size=32 is config 3's fused kernel)."""
        if precision is None:
            precision = 'f32' if model == 'mlp' else 'f64'
        lib = _native.load()
        features = np.ascontiguousarray(features, dtype=np.float64)
        labels, n_classes = labels_from_targets(targets)
        n_rows, n_features = features.shape
        if len(labels) != n_rows:
            raise ValueError('features and targets differ in length')
        cfg = make_config(n_rows, n_features, n_classes, num_envs, batch_size, max_steps,
                          precision, device, auto_reset, model, hidden)
        self.num_envs = int(num_envs)
        self.n_rows, self.n_features, self.n_classes = n_rows, n_features, n_classes
        self.batch_size = n_rows if batch_size is None else int(batch_size)
        self.max_steps = int(max_steps)
        self.precision = precision
        # hidden: one width (config 3: 64) or a tuple of widths, e.g. the
        # reference's create_neural_net default (256, 256)
        self.model = model
        self.hidden = int(hidden) if np.isscalar(hidden) else tuple(int(h) for h in hidden)
        self.device = int(device)
        self._labels = np.ascontiguousarray(labels, dtype=np.int32)
        handle = ctypes.c_void_p()
        check(lib.ce_create(ctypes.byref(cfg), features.ctypes.data, self._labels.ctypes.data,
                            ctypes.byref(handle)), 'ce_create')
        self._lib = lib
        self._h = handle
        self.act_dim = lib.ce_act_dim(handle)
        self.step_kernel = lib.ce_step_kernel(handle).decode()
        self.many_kernel = lib.ce_step_many_kernel(handle).decode()
        self.obs_dim = lib.ce_obs_dim(handle)
        view = CeOutputs()
        check(lib.ce_host_outputs(handle, ctypes.byref(view)), 'ce_host_outputs')
        E = self.num_envs
        self._host = {
            'obs': _view(view.obs, E * self.obs_dim, ctypes.c_float, np.float32,
                         (E, self.obs_dim)),
            'reward': _view(view.reward, E, ctypes.c_float, np.float32, (E,)),
            'done': _view(view.done, E, ctypes.c_uint8, np.uint8, (E,)),
            'objective': _view(view.objective, E, ctypes.c_float, np.float32, (E,)),
            'accuracy': _view(view.accuracy, E, ctypes.c_float, np.float32, (E,)),
            'episode_len': _view(view.episode_len, E, ctypes.c_int32, np.int32, (E,)),
        }
        self.seeds = [None] * E
        self.compact = False

    # ------------------------------------------------------------------ seeding
    def seed(self, seeds):
        """Seed every env (``BaseEnvironment.seed``, baseenvironment.py:20-28)."""
        if seeds is None or isinstance(seeds, (int, np.integer)):
            seeds = [seeds] * self.num_envs if seeds is None else [
                int(seeds) + i for i in range(self.num_envs)]
        seeds = [normalize_seed(s) for s in seeds]
        if len(seeds) != self.num_envs:
            raise ValueError('need one seed per env')
        arr = np.array(seeds, dtype=np.uint64)
        check(self._lib.ce_seed(self._h, arr.ctypes.data, self.num_envs), 'ce_seed')
        self.seeds = seeds
        return seeds

    # --------------------------------------------------------------- host mode
    def reset(self):
        check(self._lib.ce_reset(self._h, None, 0), 'ce_reset')
        _native.warn_stale()
        return self._host['obs'].copy()

    def step_async(self, actions):
        actions = np.ascontiguousarray(actions, dtype=np.float32)
        if actions.shape != (self.num_envs, self.act_dim):
            actions = actions.reshape(self.num_envs, self.act_dim)
        self._pending = actions   # keep alive until the H2D copy is done
        check(self._lib.ce_step_async(self._h, actions.ctypes.data, None, 0), 'ce_step_async')

    def step_wait(self):
        """Return views of the pinned outputs (valid until the next step)."""
        check(self._lib.ce_wait(self._h), 'ce_wait')
        self._pending = None
        _native.warn_stale()
        return self._host

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    # ------------------------------------------------------------- device mode
    def set_stream(self, stream_handle):
        check(self._lib.ce_set_stream(self._h, ctypes.c_void_p(stream_handle or 0)),
              'ce_set_stream')

    @staticmethod
    def _outputs(out):
        obs = out['obs_tail'] if 'obs_tail' in out else out['obs']
        return CeOutputs(obs=obs.data_ptr(),
                         reward=out['reward'].data_ptr() if 'reward' in out else None,
                         done=out['done'].data_ptr() if 'done' in out else None,
                         objective=out['objective'].data_ptr(),
                         accuracy=out['accuracy'].data_ptr(),
                         episode_len=out['episode_len'].data_ptr())

    def set_compact_outputs(self, on=True):
        """Device-pointer calls write the compact form (``ce_set_compact_outputs``):
        ``obs_tail`` = obs[:, P:] (the wght_hist block obs[:, :P] is
        identically 0, optimize.py:84-86), no ``done`` (done == episode_len
        >= max_steps) and no ``reward`` (= -objective when B = N):
        96 B per env at P = 20.  ``derived_fields`` rebuilds all three.  Raises
        ``NativeEngineError`` (CE_EUNSUPPORTED) unless this engine runs the
        two-class full-batch float64 kernel."""
        check(self._lib.ce_set_compact_outputs(self._h, 1 if on else 0), 'ce_set_compact_outputs')
        self.compact = bool(on)

    def output_fields(self):
        """(name, torch dtype, rows per env, trailing shape) of the step outputs
        as the engine writes them (full or compact form)."""
        import torch
        if self.compact:
            return [('obs_tail', torch.float32, 1, (self.act_dim + 1,)),
                    ('objective', torch.float32, 1, ()),
                    ('accuracy', torch.float32, 1, ()),
                    ('episode_len', torch.int32, 1, ())]
        return [('obs', torch.float32, 1, (self.obs_dim,)),
                ('reward', torch.float32, 1, ()),
                ('done', torch.uint8, 1, ()),
                ('objective', torch.float32, 1, ()),
                ('accuracy', torch.float32, 1, ()),
                ('episode_len', torch.int32, 1, ())]

    def derived_fields(self):
        """Fields the compact form leaves out, as functions of the fields it
        stores (name -> fn(fields) -> tensor): the full obs rows (zeros for
        the wght_hist block), done (episode_len >= max_steps) and reward
        (-objective).  The last is bit-exact because the compact form exists
        only on the two-class full-batch kernel, where B == N makes the
        minibatch loss and the full-data objective the same float64 number
        (optimize.py:91,94-97) and float32(-x) == -float32(x)."""
        if not self.compact:
            return {}
        return compact_derived(self.act_dim, self.max_steps)

    def alloc_device_outputs(self, torch_device=None):
        import torch
        dev = torch_device or torch.device('cuda', self.device)
        return {name: torch.empty((self.num_envs * rows,) + tail, dtype=dtype, device=dev)
                for name, dtype, rows, tail in self.output_fields()}

    def _check_device_tensors(self, actions, out, steps=1, strided=False):
        import torch
        if actions.dtype != torch.float32 or not actions.is_contiguous():
            raise ValueError('actions must be a contiguous float32 device tensor')
        if actions.numel() < steps * self.num_envs * self.act_dim:
            raise ValueError('actions tensor too small')
        for key, t in out.items():
            if not t.is_contiguous():
                raise ValueError('output %s must be contiguous' % key)
            if strided and t.data_ptr() % 16:
                raise ValueError('output %s must be 16-byte aligned' % key)
        if self.compact:
            if 'obs_tail' not in out or out['obs_tail'].numel() != self.num_envs * (self.act_dim + 1):
                raise ValueError('compact outputs need obs_tail of [E][P + 1]')
        elif 'obs' not in out or out['obs'].numel() != self.num_envs * self.obs_dim:
            raise ValueError('obs output has the wrong size')

    def reset_device(self, out):
        o = self._outputs(out)
        check(self._lib.ce_reset(self._h, ctypes.byref(o), _native.CE_PTR_DEVICE),
              'ce_reset')
        _native.warn_stale()

    def step_device(self, actions, out):
        """Stream-ordered step from a device action tensor into device outputs."""
        self._check_device_tensors(actions, out)
        o = self._outputs(out)
        check(self._lib.ce_step_async(self._h, actions.data_ptr(), ctypes.byref(o),
                                      _native.CE_PTR_DEVICE), 'ce_step_async')

    def step_many_device(self, k, actions, out, per_step_actions=True):
        """k stream-ordered steps (one hipGraph); actions [k][E][P] or [E][P]."""
        self._check_device_tensors(actions, out, k if per_step_actions else 1)
        stride = self.num_envs * self.act_dim if per_step_actions else 0
        o = self._outputs(out)
        check(self._lib.ce_step_many(self._h, int(k), actions.data_ptr(), stride,
                                     ctypes.byref(o)), 'ce_step_many')

    def many_runner(self, k, actions, out, per_step_actions=True):
        """step_many_device bound once: the tensors are checked and the
        argument struct built here, and the returned callable issues the k
        steps with one foreign call (a training loop replaying fixed device
        buffers pays no per-call Python validation).  The callable holds
        references to `actions` and `out`."""
        self._check_device_tensors(actions, out, k if per_step_actions else 1)
        stride = self.num_envs * self.act_dim if per_step_actions else 0
        o = self._outputs(out)
        fn, h, ap, ref, kk = self._lib.ce_step_many, self._h, actions.data_ptr(), ctypes.byref(o), int(k)

        def run():
            rc = fn(h, kk, ap, stride, ref)
            if rc:
                check(rc, 'ce_step_many')
        run.keep = (actions, out, o)
        return run

    def prepare_many_device(self, k, actions, out, per_step_actions=True):
        """Instantiate (and upload) the k-step hipGraph without running it."""
        self._check_device_tensors(actions, out, k if per_step_actions else 1)
        stride = self.num_envs * self.act_dim if per_step_actions else 0
        o = self._outputs(out)
        check(self._lib.ce_step_many_prepare(self._h, int(k), actions.data_ptr(), stride,
                                             ctypes.byref(o)), 'ce_step_many_prepare')

    def wait(self):
        check(self._lib.ce_wait(self._h), 'ce_wait')
        _native.warn_stale()

    # ------------------------------------------------- K steps in one launch
    def set_persistent(self, on=True):
        """K-step calls (step_many_device, rollout_device) as ONE launch of
        the persistent kernel where this engine has one (``many_kernel``
        names it), or one launch per step (on=False, the A/B form)."""
        check(self._lib.ce_set_persistent(self._h, 1 if on else 0), 'ce_set_persistent')
        self.many_kernel = self._lib.ce_step_many_kernel(self._h).decode()

    @property
    def persistent(self):
        return self.many_kernel.startswith('optimize_lr_persist')

    def alloc_rollout(self, k, torch_device=None):
        """A [k] array of output records for ``rollout_device``: one byte
        buffer whose record t holds step t's fields (256-B aligned segments).
        Returns (fields, record_bytes): fields maps each output name to a
        (k, E, ...) view of the buffer."""
        import torch
        from custom_envs_amd.distributed import PackedLayout
        lay = PackedLayout(self.output_fields(), self.num_envs)
        buf = torch.zeros(int(k) * lay.nbytes, dtype=torch.uint8,
                          device=torch_device or torch.device('cuda', self.device))
        fields = lay.chunk_views(buf, self.num_envs, int(k))
        fields['_buffer'] = buf
        return fields, lay.nbytes

    def rollout_device(self, k, actions, fields, record_bytes, per_step_actions=True):
        """k stream-ordered steps keeping every step's outputs: step t reads
        actions[t] and writes record t of ``fields`` (``alloc_rollout``)
        (``ce_step_many_strided``).  One launch where ``persistent``.
        ``fields`` must hold at least k records of ``record_bytes`` each
        (``check_rollout``)."""
        first = check_rollout(self.output_fields(), self.num_envs, k, actions, self.num_envs * self.act_dim,
                              fields, record_bytes, per_step_actions)
        self._check_device_tensors(actions, first, k if per_step_actions else 1, strided=True)
        stride = self.num_envs * self.act_dim if per_step_actions else 0
        o = self._outputs(first)
        check(self._lib.ce_step_many_strided(self._h, int(k), actions.data_ptr(), stride,
                                             ctypes.byref(o), int(record_bytes)),
              'ce_step_many_strided')

    # ------------------------------------------- closed loop: policy + env x K
    def alloc_policy_rollout(self, k, policy):
        """The buffers of ``rollout_policy``: (fields, record_bytes) as
        ``alloc_rollout`` and (policy_fields, policy_record_bytes) as
        ``policy.alloc_outputs(rows, k)``, returned as one 4-tuple."""
        fields, rec = self.alloc_rollout(k)
        pfields, prec = policy.alloc_outputs(self.num_envs, k)
        return fields, rec, pfields, prec

    def rollout_policy(self, k, policy, obs0, noise, fields, record_bytes, policy_fields,
                       policy_record_bytes=None, normalizer=None):
        """A K-step closed-loop rollout as ONE foreign call
        (``ce_rollout_policy``): for t < k, on the engine's stream, the policy
        (``custom_envs_amd.policy.MlpPolicy``) reads ``obs0`` (t = 0) or
        ``fields['obs'][t - 1]`` and writes ``policy_fields[...][t]``, then the
        env steps with ``policy_fields['env_action'][t]`` -- the kernel
        ``step_device`` launches -- and writes ``fields[...][t]``.  ``noise``:
        ``[>= k][E][A]`` N(0,1) draws, None for the deterministic policy, or a
        ``rng.DeviceRng``: step t's noise is its draw ``t + step`` formed in the
        policy kernel (``ce_rollout_policy_rng``; the caller advances it).
        Needs the full output form.  Every tensor is validated first
        (``policy.validate_rollout``).  ``normalizer``: a
        ``vecnormalize.NormalizedRollout`` whose slot 0 is ``obs0``: a third
        launch per step normalises record t's obs and reward into its slot
        t + 1 and record t, and the policy reads the normalised slots
        (``ce_rollout_policy_vecnorm``); ``fields`` stay raw."""
        from custom_envs_amd.policy import validate_rollout
        if self.compact:
            raise ValueError('rollout_policy needs the full output form (compact outputs are on)')
        first, prec = validate_rollout(self.output_fields(), self.num_envs, self.num_envs,
                                       self.obs_dim, self.act_dim, self.device, k, policy, obs0,
                                       noise, fields, record_bytes, policy_fields,
                                       policy_record_bytes)
        o = self._outputs(first)
        po = policy.outputs_struct({n: policy_fields[n][0] for n in
                                    ('action', 'env_action', 'neglogp', 'value')})
        if normalizer is not None:
            from custom_envs_amd.vectorize.vecnormalize import rollout_call
            rollout_call(self._lib.ce_rollout_policy_vecnorm, 'ce_rollout_policy_vecnorm', self._h,
                         policy, normalizer, k, self.num_envs, self.obs_dim, self.act_dim,
                         self.device, noise, o, record_bytes, po, prec)
            return
        if hasattr(noise, 'row_offset'):       # a DeviceRng (validated above)
            check(self._lib.ce_rollout_policy_rng(
                self._h, policy._h, int(k), obs0.data_ptr(), noise.seed, int(noise.t),
                noise.row_offset, ctypes.byref(o), int(record_bytes), ctypes.byref(po), prec),
                'ce_rollout_policy_rng')
            return
        check(self._lib.ce_rollout_policy(
            self._h, policy._h, int(k), obs0.data_ptr(),
            None if noise is None else noise.data_ptr(), self.num_envs * self.act_dim,
            ctypes.byref(o), int(record_bytes), ctypes.byref(po), prec), 'ce_rollout_policy')

    def rollout_runner(self, k, actions, fields, record_bytes, per_step_actions=True):
        """rollout_device bound once (see many_runner)."""
        first = check_rollout(self.output_fields(), self.num_envs, k, actions, self.num_envs * self.act_dim,
                              fields, record_bytes, per_step_actions)
        self._check_device_tensors(actions, first, k if per_step_actions else 1, strided=True)
        stride = self.num_envs * self.act_dim if per_step_actions else 0
        o = self._outputs(first)
        fn, h, ap, ref, kk, rb = (self._lib.ce_step_many_strided, self._h, actions.data_ptr(),
                                  ctypes.byref(o), int(k), int(record_bytes))

        def run():
            rc = fn(h, kk, ap, stride, ref, rb)
            if rc:
                check(rc, 'ce_step_many_strided')
        run.keep = (actions, fields, o)
        return run

    # ------------------------------------------------------------------ state
    def get_state(self):
        E, P, N = self.num_envs, self.act_dim, self.n_rows
        st = {'weights': np.zeros((E, P)), 'grad_hist': np.zeros((E, P)),
              'loss_hist': np.zeros(E), 'step': np.zeros(E, np.int32),
              'init_weights': np.zeros((E, P))}
        if self.batch_size < N:
            st['order'] = np.zeros((E, N), np.int32)
        cst = CeState(**{k: v.ctypes.data for k, v in st.items()})
        check(self._lib.ce_get_state(self._h, ctypes.byref(cst)), 'ce_get_state')
        return st

    def set_state(self, **state):
        conv = {'weights': np.float64, 'grad_hist': np.float64, 'loss_hist': np.float64,
                'step': np.int32, 'init_weights': np.float64, 'order': np.int32}
        arrays = {k: np.ascontiguousarray(v, dtype=conv[k]) for k, v in state.items()}
        cst = CeState(**{k: v.ctypes.data for k, v in arrays.items()})
        check(self._lib.ce_set_state(self._h, ctypes.byref(cst)), 'ce_set_state')

    def close(self):
        if getattr(self, '_h', None):
            self._lib.ce_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
