"""The training loop on the device: ``PPO2``, ``A2C`` and ``DDPG`` with
stable-baselines 2.x's constructor names, ``learn``, ``predict``, ``save`` and
``load``.

A training script of the reference (run_multiagent_exp_single.py:30-54,
search_optimize_hyperparam.py:33-66) changes one import line:

    from custom_envs_amd.agents import PPO2, A2C, DDPG, MlpPolicy, ddpg

``learn`` is the loop the pieces of this package were written for: per update
one ``env.collect`` (the closed-loop rollout, ``vectorize/collect.py``) and one
learner ``update`` (``ppo2.PPO2Learner`` / ``a2c.A2CLearner``), with every
random number taken from the counter-based generator (``rng.DeviceRng``): the
policy's noise is formed inside the policy kernel, the minibatch permutations
come from the same seed, and ``predict`` has a counter of its own, so
evaluation does not disturb training's stream.  A run is a function of
``seed``, the env's own seeding and the hyper-parameters; ``save`` / ``load``
carry the parameters, the optimiser's state, ``num_timesteps`` and the
generator's position, so a resumed run continues bit for bit.

What differs from stable-baselines, on purpose:

* ``env`` is a ``GPUVecEnv`` or an engine-backed ``OptVecEnv``, bare or inside
  a ``vectorize.vecnormalize.VecNormalize`` (``PPO2`` and ``A2C``; the running
  moments are saved with its ``save_running_average``, not by ``save``); rows
  are envs x agents.  ``seed`` seeds the agent (initial parameters, noise,
  permutations), not the env, which is seeded where it is built.
* ``learn`` resets the env only when it has no observation to start from, so
  a second ``learn`` (``reset_num_timesteps=False``) continues the episodes.
* ``policy_kwargs`` takes ``net_arch=[dict(pi=[...], vf=[...])]`` with equal
  widths (the device policy is two separate tanh networks of one shape).
* ``save`` writes one ``.npz`` through ``np.savez`` (no pickle); ``load`` reads
  that file only, not stable-baselines' own pickles.  A callable
  ``learning_rate`` / ``cliprange`` is not stored: pass it to ``load`` again.
* A2C's ``lr_schedule`` is ``'constant'`` or ``'linear'``.  ``'linear'``
  follows stable-baselines' ``Scheduler`` as remembered (stable-baselines is
  not installed where this was written, so it was not compared against it):
  the scheduler is evaluated once per batch row, so update ``u`` (1-based)
  uses ``lr * (1 - (u * n_batch - 1) / total_timesteps)``.
* ``MlpLstmPolicy`` is not here.

``diagnostics=True`` (every algorithm) adds stable-baselines' training log:
``learn`` keeps ``ep_info_buf``, the last 100 episodes the env's device monitor
(``utils_logging.DeviceVecMonitor``) finished during the call, PPO2 and A2C
compute ``explained_variance`` of each update's values and returns on the
device (``ce_explained_variance``; read back only where it is printed or
``last_diagnostics`` is read), and the log gains ``ep_rewmean``, ``eplenmean``
(NaN while the buffer is empty), ``explained_variance``, ``fps``,
``time_elapsed`` and ``total_timesteps``; ``model.last_diagnostics`` is the
same as a dict.  Without a device monitor on the env the episode entries are
absent.  After ``distribute`` the values cover this rank's rows.  The update
itself is untouched: the parameters are the bits of a run without diagnostics.

Several GPUs: every rank builds its model on its own shard of the env rows
with the same ``seed`` and calls ``model.distribute(rank, world, group,
counts)`` once, before ``learn``.  That attaches a
``distributed.GradientExchange`` to the learner, sets the generator's
``row_offset`` to ``sum(counts[:rank])`` (the noise of rank r is then the rows
``off_r ..`` of the one-rank stream) and, with ``broadcast``, sends rank 0's
parameters and optimiser state to every replica.  ``learn`` then counts
timesteps globally (``n_batch = sum(counts) * n_steps``, the same number of
updates on every rank), PPO2 permutes a rank's rows by its slice of the epoch's
key stream (``rng.permutation_numpy(seed, t, n, offset, total)``), only rank 0
prints, and a ``callback`` that returns ``False`` on any rank stops every rank
after the same update (one tiny collective per update, only when a callback
was given; an exception a callback raises on one rank is the caller's to
propagate to the others).  The replicas stay bit-identical, so ``save`` works
on any rank, and ``load`` followed by ``distribute`` at the same world
continues bit for bit.

``DDPG(ddpg.MlpPolicy, env, ...)`` (``ddpg.WideMlpPolicy`` for an env past 128
observations or 64 actions, up to 1024 -> 512) is stable-baselines' cycle: per cycle one
``env.collect_ddpg`` of ``nb_rollout_steps`` steps into the replay memory, the
action noise (``ddpg.NormalActionNoise`` / ``ddpg.OrnsteinUhlenbeckActionNoise``)
formed inside the act kernel, then one ``DDPGAgent.train`` call of
``nb_train_steps`` steps whose replay indices come from the same seed; the
train phase is skipped while the memory holds fewer than ``batch_size``
records.  What differs from stable-baselines there:

* every env row steps every rollout step, so a cycle is ``rows *
  nb_rollout_steps`` timesteps and ``learn`` runs ``total_timesteps //`` that
  many cycles (SB's ``nb_epoch_cycles`` grouping is only its logging);
* ``buffer_size`` is rounded down to a multiple of ``rows`` (a step's records
  are one slice of the ring);
* ``save(path, memory=True)`` also stores the replay memory; without it a
  loaded model starts from an empty memory, as SB's does;
* under ``distribute`` ``batch_size`` and ``buffer_size`` are per rank (as for
  stable-baselines' MPI workers): a train step is the single agent's on the
  ``world * batch_size`` rows the ranks sample from their own memories, a
  cycle trains only when every rank's memory holds ``batch_size`` records
  (decided on every rank from ``counts`` and the cycle number, without
  communication), and ``save(memory=True)`` holds that rank's memory only;
* parameter noise, layer norm, observation / return normalisation (DDPG's own,
  and a ``VecNormalize`` env), pop-art,
  ``critic_l2_reg``, ``clip_norm``, ``reward_scale != 1``,
  ``random_exploration``, ``eval_env`` and ``render`` raise ``ValueError``.
"""
import json
import os

import numpy as np

from custom_envs_amd import ddpg
from custom_envs_amd import policy as _policy
from custom_envs_amd.rng import DeviceRng


class MlpPolicy:
    """The marker stable-baselines scripts pass as ``policy``: the device-side
    actor-critic MLP (``custom_envs_amd.policy.MlpPolicy``)."""


class WideMlpPolicy:
    """The marker of the same MLP for wide shapes (obs_dim <= 1024, act_dim <=
    512: ``custom_envs_amd.policy.WideMlpPolicy`` and the wide learners): the
    reference's default 7x7-image ``Optimize-v0`` is 981 -> 490."""


class EnvSpec:
    """The shape of an env without the env: what ``load`` builds a model on
    when no env is given, and what argument checks need.  Such a model can
    ``predict`` (with a ``device``) but not ``learn``."""

    def __init__(self, rows, obs_dim, act_dim, low=None, high=None, device=None):
        self.rows, self.obs_dim, self.act_dim = int(rows), int(obs_dim), int(act_dim)
        self.low = None if low is None else np.broadcast_to(
            np.asarray(low, np.float32), (self.act_dim,)).copy()
        self.high = None if high is None else np.broadcast_to(
            np.asarray(high, np.float32), (self.act_dim,)).copy()
        self.device = None if device is None else int(device)


def env_spec(env):
    """``EnvSpec`` of a ``GPUVecEnv`` or an engine-backed ``OptVecEnv`` (rows
    are envs x agents; widths from the env's engine, bounds from its action
    space), or of a ``VecNormalize`` around one; an ``EnvSpec`` passes
    through.  Anything else: ``TypeError``."""
    if isinstance(env, EnvSpec):
        return env
    from custom_envs_amd.vectorize.vecnormalize import VecNormalize
    if isinstance(env, VecNormalize):        # the wrapped env's shape
        return env_spec(env.venv)
    from custom_envs_amd.vectorize.gpuvecenv import GPUVecEnv
    from custom_envs_amd.vectorize.optvecenv import OptVecEnv
    if isinstance(env, GPUVecEnv):
        eng = env.engine
        space = env.single_action_space
        return EnvSpec(env.num_envs, eng.obs_dim, eng.act_dim, space.low.reshape(-1),
                       space.high.reshape(-1), eng.device)
    if isinstance(env, OptVecEnv) and env.engine_backed:
        eng = env._engine
        return EnvSpec(eng.rows, 3 * eng.max_history, 1, env.action_space.low.reshape(-1),
                       env.action_space.high.reshape(-1), getattr(eng, 'device', 0))
    raise TypeError('env must be a GPUVecEnv or an engine-backed OptVecEnv (every factory the '
                    'same MultiOptLRs-v0 spec), got %s' % type(env).__name__)


def hidden_from_policy_kwargs(policy_kwargs):
    """``net_arch=[dict(pi=[...], vf=[...])]`` -> the hidden widths (default
    (64, 64)).  Unequal pi / vf widths, shared layers and other keys raise."""
    if not policy_kwargs:
        return (64, 64)
    unknown = set(policy_kwargs) - {'net_arch'}
    if unknown:
        raise ValueError('policy_kwargs takes net_arch only, got %s' % sorted(unknown))
    arch = policy_kwargs['net_arch']
    if (not isinstance(arch, (list, tuple)) or len(arch) != 1 or not isinstance(arch[0], dict)
            or set(arch[0]) != {'pi', 'vf'}):
        raise ValueError('net_arch must be [dict(pi=[...], vf=[...])] (no shared layers), got %r'
                         % (arch,))
    pi, vf = tuple(int(h) for h in arch[0]['pi']), tuple(int(h) for h in arch[0]['vf'])
    if pi != vf:
        raise ValueError('the pi and vf networks must have equal widths, got pi=%s vf=%s'
                         % (list(pi), list(vf)))
    if not pi:
        raise ValueError('net_arch needs at least one hidden layer')
    return pi


def init_params_numpy(layout, seed):
    """The initial flat float32 parameters, a function of ``seed``:
    orthogonal kernels as stable-baselines' ``ortho_init`` (gain sqrt 2 for
    hidden layers, 0.01 for the mean head, 1 for the value head), zero biases,
    ``logstd`` 0.  (The draws are NumPy's ``RandomState(seed mod 2^32)``.)"""
    rs = np.random.RandomState(int(seed) & 0xffffffff)
    flat = np.zeros(_policy.layout_size(layout), np.float32)
    for name, (off, shape) in layout.items():
        if len(shape) != 2:
            continue
        gain = {'pi/w_out': 0.01, 'vf/w_out': 1.0}.get(name, np.sqrt(2.0))
        a = rs.normal(0.0, 1.0, shape)
        u, _, vt = np.linalg.svd(a, full_matrices=False)
        q = u if u.shape == shape else vt
        flat[off:off + q.size] = (gain * q).astype(np.float32).reshape(-1)
    return flat


def linear_schedule_lr(lr, update, n_batch, total_timesteps):
    """A2C's ``lr_schedule='linear'`` at update ``update`` (1-based); see the
    module docstring."""
    return float(lr) * (1.0 - (int(update) * int(n_batch) - 1) / float(total_timesteps))


def ppo2_frac(update, n_updates):
    """PPO2's ``frac`` at update ``update`` (1-based): 1 at the first update,
    ``1 / n_updates`` at the last."""
    return 1.0 - (int(update) - 1.0) / int(n_updates)


def _constfn(value):
    return value if callable(value) else (lambda _frac, v=float(value): v)


class Distributed:
    """What ``distribute`` fixed for one replica: its rank, the world, every
    rank's env rows, this rank's first global row and the rows together."""

    def __init__(self, rank, world, counts, group=None):
        self.rank, self.world, self.counts, self.group = rank, world, list(counts), group
        self.offset, self.total = sum(self.counts[:rank]), sum(self.counts)


def ddpg_ranks_ready(counts, sizes, capacities, cycles, nb_rollout_steps, batch_size):
    """Whether a DDPG cycle trains: every rank's memory holds at least
    ``batch_size`` records after ``cycles`` more rollouts of
    ``nb_rollout_steps`` steps on top of the ``sizes`` it started from.  A
    function of what every rank knows, so every rank decides alike and none
    enters a collective alone."""
    return all(min(cap, size + int(cycles) * rows * int(nb_rollout_steps)) >= int(batch_size)
               for rows, size, cap in zip(counts, sizes, capacities))


class BaseAgent:
    """What ``PPO2`` and ``A2C`` share: the env's shape, the device policy and
    its learner, the generator, ``learn``'s loop, ``predict``, ``save`` and
    ``load``.  A subclass gives ``LEARNER``, ``OPT_INIT``, its constructor and
    ``_update``."""
    LEARNER = None
    WIDE_LEARNER = None          # the learner of ``WideMlpPolicy``
    OPT_INIT = {}                # shape-only models: block name -> fill value
    LOG_INTERVAL = 1
    diagnostics = False          # the constructor's switch (module docstring)

    def _setup(self, policy, env, kwargs, seed, verbose, policy_kwargs, learner_kwargs):
        if policy is WideMlpPolicy or policy == 'WideMlpPolicy':
            self.policy_kind = 'WideMlpPolicy'
        elif policy is MlpPolicy or policy == 'MlpPolicy':
            self.policy_kind = 'MlpPolicy'
        else:
            raise ValueError('policy must be agents.MlpPolicy or agents.WideMlpPolicy, got %r'
                             % (policy,))
        wide = self.policy_kind == 'WideMlpPolicy'
        self.hidden = hidden_from_policy_kwargs(policy_kwargs)
        self.spec = env_spec(env)
        self.env = None if isinstance(env, EnvSpec) else env
        self.kwargs = dict(kwargs, policy_kwargs=policy_kwargs, verbose=int(verbose))
        self.verbose = int(verbose)
        if seed is None:
            seed = int.from_bytes(os.urandom(8), 'little')
        self.seed = int(seed)
        self.kwargs['seed'] = self.seed
        self.n_batch = self.spec.rows * self.n_steps
        self.num_timesteps = 0
        s = self.spec
        policy_cls = _policy.WideMlpPolicy if wide else _policy.MlpPolicy
        self.policy = policy_cls(s.obs_dim, s.act_dim, self.hidden, low=s.low, high=s.high,
                                 device=s.device)
        self.learner = (self.WIDE_LEARNER if wide else self.LEARNER)(self.policy, **learner_kwargs)
        self.rng = DeviceRng(self.seed, s.device)
        self._host = None
        flat = init_params_numpy(self.policy.params_layout(), self.seed)
        if s.device is None:     # shape only: the state lives here
            self._host = {'params': flat, 'opt': dict(
                {n: np.full(flat.size, v, np.float32) for n, v in self.OPT_INIT.items()}, step=0)}
        else:
            self.learner.set_params(flat)

    # ------------------------------------------------------------- the state
    def get_parameters(self):
        """The flat float32 parameters (``policy.params_layout``), numpy."""
        if self._host is not None:
            return self._host['params'].copy()
        return self.learner.get_params()

    def set_parameters(self, flat):
        flat = np.ascontiguousarray(flat, np.float32).reshape(-1)
        if flat.size != self.policy.n_params:
            raise ValueError('got %d parameters, the policy has %d'
                             % (flat.size, self.policy.n_params))
        if self._host is not None:
            self._host['params'] = flat.copy()
        else:
            self.learner.set_params(flat)

    def get_opt_state(self):
        if self._host is not None:
            return {k: (v.copy() if hasattr(v, 'copy') else v)
                    for k, v in self._host['opt'].items()}
        return self.learner.get_opt_state()

    def set_opt_state(self, state):
        if self._host is not None:
            a, b, step = self.learner.check_opt_state(state)
            names = self.learner.OPT_BLOCKS
            self._host['opt'] = {names[0]: a.copy(), names[1]: b.copy(), 'step': step}
        else:
            self.learner.set_opt_state(state)

    # ------------------------------------------------------------- distribute
    dist = None                  # what ``distribute`` decided, a ``Distributed``

    def _exchange_target(self):
        """What the gradient exchange attaches to, and its ``counts``."""
        return self.learner, self.dist.counts

    def _check_distribute(self, counts):
        """A subclass's own refusals, for every rank, before anything is set."""

    def _is_shape_only(self):
        return self._host is not None

    def _after_distribute(self):
        pass

    def distribute(self, rank, world, group=None, counts=None, collective=None, broadcast=True):
        """Make this model rank ``rank`` of ``world`` data-parallel replicas
        (see the module docstring).  ``counts``: every rank's env rows
        (default: this env's rows on every rank); the rank's env is the rows
        ``off_r .. off_r + counts[r] - 1`` of the global batch, ``off_r =
        sum(counts[:r])``.  ``group`` / ``collective``: as
        ``distributed.GradientExchange``.  ``broadcast``: send rank 0's
        parameters (and targets) and optimiser state to every replica; needs a
        device, so a shape-only model passes ``broadcast=False`` (it can check
        arguments, not learn).  Every refusal is raised before any launch, and
        from ``counts`` alone wherever another rank would refuse.  Returns the
        exchange."""
        from custom_envs_amd.distributed import GradientExchange
        from custom_envs_amd.vectorize.vecnormalize import VecNormalize
        if isinstance(self.env, VecNormalize):
            raise NotImplementedError('distribute() with a VecNormalize env is not supported: the '
                                      'ranks\' running moments are not merged')
        if self.dist is not None:
            raise RuntimeError('distribute() was already called on this model')
        world, rank = int(world), int(rank)
        if world <= 0 or not 0 <= rank < world:
            raise ValueError('bad rank/world')
        counts = [self.spec.rows] * world if counts is None else [int(c) for c in counts]
        if len(counts) != world or min(counts) < 1:
            raise ValueError('counts must give every one of the %d ranks at least one row, got %s'
                             % (world, counts))
        if counts[rank] != self.spec.rows:
            raise ValueError('rank %d: counts says %d rows, the env has %d'
                             % (rank, counts[rank], self.spec.rows))
        if sum(counts) > 2 ** 32:
            raise ValueError('the ranks\' rows together must stay below 2^32')
        if broadcast and self._is_shape_only():
            raise ValueError('a shape-only model has no parameters on a device to broadcast: '
                             'distribute(..., broadcast=False) checks arguments only')
        self._check_distribute(counts)
        self.dist = Distributed(rank, world, counts, group)
        target, ex_counts = self._exchange_target()
        ex = self.exchange = GradientExchange(target, rank, world, group=group, counts=ex_counts,
                                              collective=collective)
        self.rng.row_offset = self.dist.offset
        self.n_batch = self.dist.total * self._steps_per_batch()
        self._after_distribute()
        if broadcast:
            ex.broadcast_params(0)
            ex.broadcast_opt_state(0)
        return ex

    def _steps_per_batch(self):
        return self.n_steps

    def _stop_everywhere(self, stop):
        """``stop`` on any rank, on every rank: one tiny collective."""
        d = self.dist
        if d is None or not (d.world > 1 and self.exchange.collective):
            return stop
        from custom_envs_amd.distributed import host_all_gather_int
        return any(host_all_gather_int(int(stop), d.world, d.group))

    # ------------------------------------------------------------------ learn
    def check_learn(self, total_timesteps):
        """``n_updates`` of a ``learn(total_timesteps)`` call (no GPU).  After
        ``distribute`` a batch is every rank's rows together."""
        total = int(total_timesteps)
        if total < self.n_batch:
            raise ValueError('total_timesteps = %d is less than one batch (rows * n_steps = %d)'
                             % (total, self.n_batch))
        return total // self.n_batch

    def learn(self, total_timesteps, callback=None, log_interval=None, reset_num_timesteps=True):
        """``total_timesteps // (rows * n_steps)`` updates; see the module
        docstring.  ``callback(locals_, globals_)`` runs after each update
        (``locals_`` holds at least ``self`` and ``update``); a return value
        of exactly ``False`` ends the loop, and an exception propagates with
        the env and the model consistent (the update is complete).  Statistics
        are read back only on logging updates with ``verbose >= 1``.  Returns
        ``self``."""
        n_updates = self.check_learn(total_timesteps)
        total_timesteps = int(total_timesteps)
        if self.env is None:
            raise RuntimeError('learn() needs an env: this model was loaded without one '
                               '(load(path, env=...))')
        log_interval = self.LOG_INTERVAL if log_interval is None else int(log_interval)
        if reset_num_timesteps:
            self.num_timesteps = 0
        env = self.env
        if getattr(env, '_last_obs', None) is None:
            env.reset()
        if self.diagnostics:
            self._diag_begin(env)
        for update in range(1, n_updates + 1):
            stats = self._update(env, update, n_updates, total_timesteps)
            self.num_timesteps += self.n_batch
            if self.diagnostics:
                self._diag_update(env)
            printing = self.dist is None or self.dist.rank == 0
            if self.verbose >= 1 and printing and log_interval > 0 \
                    and (update % log_interval == 0 or update == 1):
                self._log(update, stats)
            if callback is not None:
                if self._stop_everywhere(callback(locals(), globals()) is False):
                    break
        return self

    def _log(self, update, stats):
        last = stats[-1] if isinstance(stats, (list, tuple)) else stats
        print('| update %d | timesteps %d |' % (update, self.num_timesteps))
        for key, value in last.stats().items():
            print('| %-12s | %-12.5g |' % (key, value))
        self._log_diagnostics()

    # ------------------------------------------------------------ diagnostics
    _ev = None                   # the update's explained variance, a device scalar

    def _diag_begin(self, env):
        import time
        from collections import deque
        self.ep_info_buf = deque(maxlen=100)
        monitor = getattr(env, 'monitor', None)
        self._diag_monitor = monitor if getattr(monitor, 'on_device', False) else None
        self._diag_seen = 0 if self._diag_monitor is None else self._diag_monitor.n_finished
        self._diag_t0 = self._diag_t = time.time()
        self._diag = None

    def _diag_update(self, env):
        """After an update: the monitor's new rows into ``ep_info_buf``, the
        timing; nothing is read from the device."""
        import time
        mon = self._diag_monitor
        if mon is not None:
            new = min(mon.n_finished - self._diag_seen, len(mon.recent))
            self._diag_seen = mon.n_finished
            if new:
                self.ep_info_buf.extend(list(mon.recent)[-new:])
        now = time.time()
        rows = self.spec.rows * self._steps_per_batch()
        self._diag = {'fps': int(rows / max(now - self._diag_t, 1e-9)),
                      'time_elapsed': now - self._diag_t0,
                      'total_timesteps': self.num_timesteps}
        self._diag_t = now

    @property
    def last_diagnostics(self):
        """The last update's diagnostics as a dict (None before the first
        update of a ``diagnostics=True`` model).  Reading it copies the
        explained variance from the device."""
        if not self.diagnostics or getattr(self, '_diag', None) is None:
            return None
        out = {}
        if self._diag_monitor is not None:
            buf = self.ep_info_buf
            out['ep_rewmean'] = float(np.mean([e['r'] for e in buf])) if buf else float('nan')
            out['eplenmean'] = float(np.mean([e['l'] for e in buf])) if buf else float('nan')
        if self._ev is not None:
            out['explained_variance'] = float(self._ev.item())
        out.update(self._diag)
        return out

    def _log_diagnostics(self):
        for key, value in (self.last_diagnostics or {}).items():
            print('| %-18s | %-12.5g |' % (key, value))

    def _explained_variance(self, values, returns):
        from custom_envs_amd.utils.utils_logging import explained_variance_device
        self._ev = explained_variance_device(values, returns, out=self._ev)

    # ---------------------------------------------------------------- predict
    def predict(self, observation, state=None, mask=None, deterministic=False):
        """``(actions, None)``: the policy's action for ``observation``
        (numpy or a device tensor, ``[rows][D]`` or ``[D]``), clipped to the
        action space; numpy in, numpy out.  Stochastic draws use the
        generator's ``PREDICT`` stream and its own counter."""
        import torch
        if self.policy._h is None:
            raise RuntimeError('predict() needs a device: this model holds the shape only')
        dev = torch.device('cuda', self.policy.device)
        as_numpy = not torch.is_tensor(observation)
        if as_numpy:
            obs = torch.from_numpy(np.ascontiguousarray(observation, dtype=np.float32)).to(dev)
        else:
            obs = observation.to(dev, torch.float32).contiguous()
        single = obs.dim() == 1
        if single:
            obs = obs[None]
        if obs.dim() != 2 or obs.shape[1] != self.spec.obs_dim:
            raise ValueError('observation must have shape [rows][%d] or [%d], got %s'
                             % (self.spec.obs_dim, self.spec.obs_dim, tuple(observation.shape)))
        noise = None if deterministic else self.rng.predict_normal(obs.shape[0], self.spec.act_dim)
        actions = self.policy.forward_device(obs, noise)['env_action']
        if single:
            actions = actions[0]
        if as_numpy:
            actions = actions.cpu().numpy()
        return actions, None

    # ------------------------------------------------------------ save / load
    def _meta(self):
        kwargs = {}
        for key, value in self.kwargs.items():
            kwargs[key] = {'callable': True} if callable(value) else value
        s = self.spec
        return {'format': 1, 'algorithm': type(self).__name__, 'policy': self.policy_kind,
                'kwargs': kwargs,
                'rows': s.rows, 'obs_dim': s.obs_dim, 'act_dim': s.act_dim,
                'low': None if s.low is None else [float(v) for v in s.low],
                'high': None if s.high is None else [float(v) for v in s.high],
                'hidden': list(self.hidden), 'n_params': int(self.policy.n_params),
                'opt_blocks': list(self.learner.OPT_BLOCKS)}

    def save(self, save_path):
        """One ``.npz`` (``np.savez``; a path without the suffix gets it): a
        JSON string of the constructor arguments and shapes, the flat
        parameters, the optimiser's state, ``num_timesteps`` and the
        generator's state."""
        opt = self.get_opt_state()
        g = self.rng.state()
        arrays = {'meta': np.array(json.dumps(self._meta())), 'params': self.get_parameters(),
                  'opt_step': np.array(opt['step'], np.int64),
                  'num_timesteps': np.array(self.num_timesteps, np.int64),
                  'rng': np.array([g['seed'], g['row_offset'], g['t'], g['epoch'],
                                   g['predict_t']], np.uint64)}
        for name in self.learner.OPT_BLOCKS:
            arrays['opt_' + name] = opt[name]
        np.savez(save_path, **arrays)

    @classmethod
    def _read(cls, load_path, env, device, overrides):
        """(arrays, meta, constructor kwargs, env or the saved shapes'
        ``EnvSpec``) of a saved file of this algorithm."""
        if isinstance(load_path, (str, os.PathLike)) and not os.path.exists(load_path) \
                and os.path.exists(str(load_path) + '.npz'):
            load_path = str(load_path) + '.npz'
        with np.load(load_path, allow_pickle=False) as data:
            data = {k: data[k] for k in data.files}
        meta = json.loads(str(data['meta']))
        if meta.get('algorithm') != cls.__name__:
            raise ValueError('the file holds a %s model, not a %s'
                             % (meta.get('algorithm'), cls.__name__))
        kwargs = dict(meta['kwargs'])
        kwargs.update(overrides)
        for key, value in kwargs.items():
            if isinstance(value, dict) and value.get('callable'):
                raise ValueError('%s was a callable and is not stored: pass it to load()' % key)
        if env is None:
            if device == 'auto':
                import torch
                device = 0 if torch.cuda.is_available() else None
            env = EnvSpec(meta['rows'], meta['obs_dim'], meta['act_dim'], meta['low'],
                          meta['high'], device)
        return data, meta, kwargs, env

    @classmethod
    def load(cls, load_path, env=None, device='auto', **overrides):
        """The model ``save`` wrote, from a path (with or without ``.npz``) or
        an open binary file.  ``env``: the env to go on learning with; None
        builds the model on the saved shapes, which can ``predict`` (on
        ``device``; ``'auto'``: cuda:0 when there is one, else the shape only)
        but not ``learn``.  ``overrides`` replace constructor arguments (a
        callable ``learning_rate`` / ``cliprange`` must be given again)."""
        data, meta, kwargs, env = cls._read(load_path, env, device, overrides)
        # a file from before the wide policy names none: MlpPolicy
        model = cls(meta.get('policy', 'MlpPolicy'), env, **kwargs)
        s = model.spec
        if (s.obs_dim, s.act_dim, list(model.hidden)) != (meta['obs_dim'], meta['act_dim'],
                                                          meta['hidden']):
            raise ValueError('the env maps %d -> %d, the saved model %d -> %d (hidden %s)'
                             % (s.obs_dim, s.act_dim, meta['obs_dim'], meta['act_dim'],
                                meta['hidden']))
        model.set_parameters(data['params'])
        opt = {name: data['opt_' + name] for name in meta['opt_blocks']}
        opt['step'] = int(data['opt_step'])
        model.set_opt_state(opt)
        model.num_timesteps = int(data['num_timesteps'])
        g = [int(v) for v in data['rng']]
        model.rng.set_state({'seed': g[0], 'row_offset': g[1], 't': g[2], 'epoch': g[3],
                             'predict_t': g[4]})
        model.seed = g[0]
        return model


class PPO2(BaseAgent):
    """stable-baselines 2.x ``PPO2`` on the device (see the module
    docstring).  ``learning_rate`` and ``cliprange`` are floats or callables
    of ``frac`` (1 at the first update, falling to ``1 / n_updates``); with a
    callable ``cliprange`` give ``cliprange_vf`` explicitly (the value clip
    is fixed per learner)."""
    OPT_INIT = {'m': 0.0, 'v': 0.0}
    LOG_INTERVAL = 1

    def __init__(self, policy, env, gamma=0.99, n_steps=128, ent_coef=0.01, learning_rate=2.5e-4,
                 vf_coef=0.5, max_grad_norm=0.5, lam=0.95, nminibatches=4, noptepochs=4,
                 cliprange=0.2, cliprange_vf=None, verbose=0, seed=None, policy_kwargs=None,
                 diagnostics=False):
        from custom_envs_amd.ppo2 import PPO2Learner, WidePPO2Learner
        self.LEARNER, self.WIDE_LEARNER = PPO2Learner, WidePPO2Learner
        self.diagnostics = bool(diagnostics)
        self.n_steps, self.nminibatches = int(n_steps), int(nminibatches)
        self.noptepochs = int(noptepochs)
        if self.n_steps < 1 or self.nminibatches < 1 or self.noptepochs < 1:
            raise ValueError('n_steps, nminibatches and noptepochs must be >= 1')
        if callable(cliprange) and cliprange_vf is None:
            raise ValueError('a callable cliprange needs an explicit cliprange_vf (the value '
                             'clip is fixed per learner; negative: none)')
        self.learning_rate, self.cliprange = _constfn(learning_rate), _constfn(cliprange)
        kwargs = dict(gamma=gamma, n_steps=self.n_steps, ent_coef=ent_coef,
                      learning_rate=learning_rate, vf_coef=vf_coef, max_grad_norm=max_grad_norm,
                      lam=lam, nminibatches=self.nminibatches, noptepochs=self.noptepochs,
                      cliprange=cliprange, cliprange_vf=cliprange_vf)
        self._setup(policy, env, kwargs, seed, verbose, policy_kwargs, dict(
            gamma=gamma, lam=lam, cliprange=float(self.cliprange(1.0)), cliprange_vf=cliprange_vf,
            ent_coef=ent_coef, vf_coef=vf_coef, max_grad_norm=max_grad_norm,
            lr=float(self.learning_rate(1.0))))
        if self.n_batch % self.nminibatches:
            raise ValueError('rows * n_steps = %d rows do not split into %d minibatches'
                             % (self.n_batch, self.nminibatches))

    def _check_distribute(self, counts):
        for r, c in enumerate(counts):
            if (self.n_steps * c) % self.nminibatches:
                raise ValueError('rank %d: rows * n_steps = %d rows do not split into %d '
                                 'minibatches' % (r, self.n_steps * c, self.nminibatches))

    def _update(self, env, update, n_updates, total_timesteps):
        frac = ppo2_frac(update, n_updates)
        result = env.collect(self.policy, self.n_steps, noise=self.rng)
        if self.dist is None:
            perms = [self.rng.permutation(self.n_batch) for _ in range(self.noptepochs)]
        else:       # this rank's slice of the epoch's keys, drawn at the global length
            d, k = self.dist, self.n_steps
            perms = [self.rng.permutation(k * self.spec.rows, offset=k * d.offset,
                                          total=k * d.total) for _ in range(self.noptepochs)]
        stats = self.learner.update(result, noptepochs=self.noptepochs,
                                    nminibatches=self.nminibatches,
                                    lr=float(self.learning_rate(frac)),
                                    cliprange=float(self.cliprange(frac)), perms=perms)
        if self.diagnostics:     # the returns the update's GAE left
            self._explained_variance(result['values'], self.learner.last_returns)
        return stats


class A2C(BaseAgent):
    """stable-baselines 2.x ``A2C`` on the device (see the module docstring):
    ``lr_schedule`` is ``'constant'`` or ``'linear'``; other schedules
    raise."""
    OPT_INIT = {'ms': 1.0, 'mom': 0.0}
    LOG_INTERVAL = 100

    def __init__(self, policy, env, gamma=0.99, n_steps=5, vf_coef=0.25, ent_coef=0.01,
                 max_grad_norm=0.5, learning_rate=7e-4, alpha=0.99, epsilon=1e-5,
                 lr_schedule='constant', verbose=0, seed=None, policy_kwargs=None,
                 diagnostics=False):
        from custom_envs_amd.a2c import A2CLearner, WideA2CLearner
        self.LEARNER, self.WIDE_LEARNER = A2CLearner, WideA2CLearner
        self.diagnostics = bool(diagnostics)
        self.n_steps = int(n_steps)
        if self.n_steps < 1:
            raise ValueError('n_steps must be >= 1')
        if lr_schedule not in ('constant', 'linear'):
            raise ValueError("lr_schedule must be 'constant' or 'linear', got %r" % (lr_schedule,))
        if callable(learning_rate):
            raise ValueError('A2C takes a float learning_rate and an lr_schedule')
        self.lr_schedule, self.learning_rate = lr_schedule, float(learning_rate)
        kwargs = dict(gamma=gamma, n_steps=self.n_steps, vf_coef=vf_coef, ent_coef=ent_coef,
                      max_grad_norm=max_grad_norm, learning_rate=self.learning_rate, alpha=alpha,
                      epsilon=epsilon, lr_schedule=lr_schedule)
        self._setup(policy, env, kwargs, seed, verbose, policy_kwargs, dict(
            gamma=gamma, ent_coef=ent_coef, vf_coef=vf_coef, max_grad_norm=max_grad_norm,
            lr=self.learning_rate, alpha=alpha, eps=epsilon))

    def lr_at(self, update, total_timesteps):
        if self.lr_schedule == 'constant':
            return self.learning_rate
        return linear_schedule_lr(self.learning_rate, update, self.n_batch, total_timesteps)

    def _update(self, env, update, n_updates, total_timesteps):
        result = env.collect(self.policy, self.n_steps, noise=self.rng)
        if self.diagnostics:     # the update keeps its returns to itself: one more scan
            self._explained_variance(result['values'], self.learner.returns(result))
        return self.learner.update(result, lr=self.lr_at(update, total_timesteps))


def ddpg_hidden_from_policy_kwargs(policy_kwargs):
    """``dict(layers=[...])`` -> the hidden widths (default (64, 64));
    ``layer_norm`` and other keys raise."""
    if not policy_kwargs:
        return (64, 64)
    if policy_kwargs.get('layer_norm'):
        raise ValueError('layer_norm is not supported (ddpg.py: out of scope)')
    unknown = set(policy_kwargs) - {'layers', 'layer_norm'}
    if unknown:
        raise ValueError('policy_kwargs takes layers only, got %s' % sorted(unknown))
    layers = policy_kwargs.get('layers')
    if layers is None:
        return (64, 64)
    hidden = tuple(int(h) for h in layers)
    if not hidden:
        raise ValueError('layers needs at least one hidden layer')
    return hidden


class DDPG(BaseAgent):
    """stable-baselines 2.x ``DDPG`` on the device (see the module docstring
    and ``custom_envs_amd.ddpg``).  ``nb_eval_steps``, ``memory_limit``,
    ``memory_policy``, ``param_noise_adaption_interval``, ``return_range`` and
    ``render_eval`` are accepted and ignored."""
    LOG_INTERVAL = 1
    # what ddpg.py lists as out of scope: keyword -> its stable-baselines default
    REFUSED = {'param_noise': None, 'normalize_observations': False, 'normalize_returns': False,
               'enable_popart': False, 'critic_l2_reg': 0.0, 'clip_norm': None,
               'reward_scale': 1.0, 'random_exploration': 0.0, 'eval_env': None, 'render': False}

    def __init__(self, policy, env, gamma=0.99, memory_policy=None, eval_env=None,
                 nb_train_steps=50, nb_rollout_steps=100, nb_eval_steps=100, param_noise=None,
                 action_noise=None, normalize_observations=False, tau=0.001, batch_size=128,
                 param_noise_adaption_interval=50, normalize_returns=False, enable_popart=False,
                 observation_range=(-5.0, 5.0), critic_l2_reg=0.0,
                 return_range=(-np.inf, np.inf), actor_lr=1e-4, critic_lr=1e-3, clip_norm=None,
                 reward_scale=1.0, render=False, render_eval=False, memory_limit=None,
                 buffer_size=50000, random_exploration=0.0, verbose=0, seed=None,
                 policy_kwargs=None, diagnostics=False):
        self.diagnostics = bool(diagnostics)
        from custom_envs_amd.vectorize.vecnormalize import VecNormalize
        if isinstance(env, VecNormalize):
            raise ValueError('DDPG on a VecNormalize env is not supported (collect_ddpg has no '
                             'normalised form)')
        self.policy_kind = ddpg.policy_kind(policy)
        if self.policy_kind is None:
            if getattr(policy, '__name__', policy) == 'LnMlpPolicy':
                raise ValueError('layer_norm (LnMlpPolicy) is not supported')
            raise ValueError('policy must be ddpg.MlpPolicy or ddpg.WideMlpPolicy, got %r'
                             % (policy,))
        given = dict(param_noise=param_noise, normalize_observations=normalize_observations,
                     normalize_returns=normalize_returns, enable_popart=enable_popart,
                     critic_l2_reg=critic_l2_reg, clip_norm=clip_norm, reward_scale=reward_scale,
                     random_exploration=random_exploration, eval_env=eval_env, render=render)
        for key, default in self.REFUSED.items():
            value = given[key]
            same = (value is None) if default is None else \
                (value is not None and not callable(value) and value == default)
            if not same:
                raise ValueError('%s=%r is not supported: only stable-baselines\' default %r '
                                 '(ddpg.py: out of scope)' % (key, value, default))
        if action_noise is not None and not isinstance(action_noise, ddpg.ActionNoise):
            raise ValueError('action_noise must be a ddpg.NormalActionNoise, a '
                             'ddpg.OrnsteinUhlenbeckActionNoise or None, got %r' % (action_noise,))
        self.hidden = ddpg_hidden_from_policy_kwargs(policy_kwargs)
        self.spec = s = env_spec(env)
        self.env = None if isinstance(env, EnvSpec) else env
        self.verbose = int(verbose)
        if seed is None:
            seed = int.from_bytes(os.urandom(8), 'little')
        self.seed = int(seed)
        self.nb_train_steps, self.nb_rollout_steps = int(nb_train_steps), int(nb_rollout_steps)
        self.batch_size = int(batch_size)
        if self.nb_train_steps < 1 or self.nb_rollout_steps < 1 or self.batch_size < 1:
            raise ValueError('nb_train_steps, nb_rollout_steps and batch_size must be >= 1')
        self.buffer_size = int(buffer_size) // s.rows * s.rows
        if self.buffer_size < max(s.rows, self.batch_size):
            raise ValueError('buffer_size = %d rounds down to %d records (a multiple of the %d '
                             'rows a step writes), which must be at least max(rows, batch_size) '
                             '= %d' % (int(buffer_size), self.buffer_size, s.rows,
                                       max(s.rows, self.batch_size)))
        self.action_noise = action_noise
        if action_noise is not None:
            action_noise.params(s.act_dim)
        self.kwargs = dict(
            gamma=float(gamma), nb_train_steps=self.nb_train_steps,
            nb_rollout_steps=self.nb_rollout_steps, tau=float(tau), batch_size=self.batch_size,
            observation_range=[float(observation_range[0]), float(observation_range[1])],
            actor_lr=float(actor_lr), critic_lr=float(critic_lr), buffer_size=int(buffer_size),
            verbose=self.verbose, seed=self.seed, policy_kwargs=policy_kwargs)
        self.n_batch = s.rows * self.nb_rollout_steps        # timesteps per cycle
        self.num_timesteps = 0
        scale = 1.0 if s.low is None else np.abs(s.low)
        self.agent = ddpg.AGENTS[self.policy_kind](
            s.obs_dim, s.act_dim, self.hidden, scale=scale, gamma=gamma, tau=tau,
            actor_lr=actor_lr, critic_lr=critic_lr, obs_range=observation_range, device=s.device)
        self.memory = ddpg.ReplayMemory(self.buffer_size, s.rows, s.obs_dim, s.act_dim,
                                        device=s.device)
        self.rng = DeviceRng(self.seed, s.device)
        self.agent.set_params(ddpg.init_params_numpy(s.obs_dim, s.act_dim, self.hidden,
                                                     self.seed & 0xffffffff))

    # ------------------------------------------------------------- distribute
    def _is_shape_only(self):
        return self.agent._h is None

    def _steps_per_batch(self):
        return self.nb_rollout_steps

    def _exchange_target(self):
        # a train step's rows are batch_size on every rank: equal shares
        return self.agent, None

    def capacities(self, counts):
        """Every rank's memory capacity: ``buffer_size`` rounded down to a
        multiple of its rows, as the constructor does for this rank's."""
        return [int(self.kwargs['buffer_size']) // c * c for c in counts]

    def _check_distribute(self, counts):
        for r, (c, cap) in enumerate(zip(counts, self.capacities(counts))):
            if cap < max(c, self.batch_size):
                raise ValueError('rank %d: buffer_size rounds down to %d records, which must be '
                                 'at least max(rows, batch_size) = %d'
                                 % (r, cap, max(c, self.batch_size)))
        state = getattr(self.action_noise, 'get_state', lambda: None)()
        if state is not None and state[0].shape[0] != self.spec.rows:
            raise ValueError('the Ornstein-Uhlenbeck state holds %d rows, this rank\'s env %d'
                             % (state[0].shape[0], self.spec.rows))

    def _after_distribute(self):
        # every rank's records at this point: what the train / skip decision
        # of every later cycle starts from
        d = self.dist
        if d.world > 1 and self.exchange.collective:
            from custom_envs_amd.distributed import host_all_gather_int
            self._sizes0 = host_all_gather_int(self.memory.size, d.world, d.group)
        else:
            self._sizes0 = [self.memory.size if r == d.rank else 0 for r in range(d.world)]
        self._cycles = 0

    def trains_after(self, cycles):
        """Whether the train phase runs after ``cycles`` rollouts since
        ``distribute`` (``ddpg_ranks_ready``; no GPU, no communication)."""
        d = self.dist
        return ddpg_ranks_ready(d.counts, self._sizes0, self.capacities(d.counts), cycles,
                                self.nb_rollout_steps, self.batch_size)

    # ------------------------------------------------------------- the state
    def get_parameters(self, target=False):
        """The flat float32 online (``target``: target) parameters
        (``ddpg.params_layout``), numpy."""
        return self.agent.get_params(target=target)

    def set_parameters(self, flat, target=None):
        """The online parameters, copied into the targets too unless
        ``target`` (a flat vector) gives those."""
        self.agent.set_params(flat)
        if target is not None:
            self.agent.set_params(target, target_only=True)

    def get_opt_state(self):
        return self.agent.get_opt_state()

    def set_opt_state(self, state):
        self.agent.set_opt_state(state)

    # ------------------------------------------------------------------ learn
    def check_learn(self, total_timesteps):
        """The cycles of a ``learn(total_timesteps)`` call (no GPU)."""
        total = int(total_timesteps)
        if total < self.n_batch:
            raise ValueError('total_timesteps = %d is less than one cycle (rows * '
                             'nb_rollout_steps = %d)' % (total, self.n_batch))
        return total // self.n_batch

    def _noise(self):
        return None if self.action_noise is None else (self.action_noise, self.rng)

    def _update(self, env, update, n_updates, total_timesteps):
        """One cycle: the rollout into the memory, then the train phase
        (skipped while the memory cannot fill a batch: SB's ``can_sample``).
        Returns the last train step's ``ddpg.Stats`` or None."""
        env.collect_ddpg(self.agent, self.memory, self.nb_rollout_steps, noise=self._noise())
        if self.dist is not None:
            self._cycles += 1
            ready = self.trains_after(self._cycles)
        else:
            ready = self.memory.size >= self.batch_size
        if not ready:
            return None
        stats = self.agent.train(self.memory, self.nb_train_steps, self.batch_size, self.rng)
        return ddpg.Stats(stats[-1])

    def _log(self, update, stats):
        if stats is None:
            print('| cycle %d | timesteps %d | memory %d < batch_size |'
                  % (update, self.num_timesteps, self.memory.size))
            self._log_diagnostics()
            return
        super()._log(update, stats)

    # ---------------------------------------------------------------- predict
    def predict(self, observation, state=None, mask=None, deterministic=True):
        """``(env_action, None)`` for ``observation`` (numpy or a device
        tensor, ``[rows][D]`` or ``[D]``); numpy in, numpy out.  With
        ``deterministic=False`` a ``NormalActionNoise`` is drawn on the
        generator's ``PREDICT`` stream and its own counter (training's
        streams are untouched); without a noise object the action is the
        deterministic one; Ornstein-Uhlenbeck noise raises (its state belongs
        to training)."""
        import torch
        if self.agent._h is None:
            raise RuntimeError('predict() needs a device: this model holds the shape only')
        noisy = not deterministic and self.action_noise is not None
        if noisy and not isinstance(self.action_noise, ddpg.NormalActionNoise):
            raise ValueError('a stochastic predict() with Ornstein-Uhlenbeck noise is not '
                             'supported: the process state belongs to training')
        dev = torch.device('cuda', self.agent.device)
        as_numpy = not torch.is_tensor(observation)
        if as_numpy:
            obs = torch.from_numpy(np.ascontiguousarray(observation, dtype=np.float32)).to(dev)
        else:
            obs = observation.to(dev, torch.float32).contiguous()
        single = obs.dim() == 1
        if single:
            obs = obs[None]
        if obs.dim() != 2 or obs.shape[1] != self.spec.obs_dim:
            raise ValueError('observation must have shape [rows][%d] or [%d], got %s'
                             % (self.spec.obs_dim, self.spec.obs_dim, tuple(observation.shape)))
        noise = None
        if noisy:
            mean, sigma = (torch.from_numpy(v).to(dev)
                           for v in self.action_noise.params(self.spec.act_dim))
            noise = mean + sigma * self.rng.predict_normal(obs.shape[0], self.spec.act_dim)
        actions = self.agent.act(obs, noise)['env_action']
        if single:
            actions = actions[0]
        if as_numpy:
            actions = actions.cpu().numpy()
        return actions, None

    # ------------------------------------------------------------ save / load
    def _meta(self):
        s = self.spec
        return {'format': 1, 'algorithm': type(self).__name__, 'policy': self.policy_kind,
                'kwargs': self.kwargs,
                'action_noise': None if self.action_noise is None
                else self.action_noise.describe(),
                'rows': s.rows, 'obs_dim': s.obs_dim, 'act_dim': s.act_dim,
                'low': None if s.low is None else [float(v) for v in s.low],
                'high': None if s.high is None else [float(v) for v in s.high],
                'hidden': list(self.hidden), 'n_params': int(self.agent.n_params),
                'opt_blocks': list(self.agent.OPT_BLOCKS)}

    def save(self, save_path, memory=False):
        """One ``.npz`` (``np.savez``, no pickle): a JSON string of the
        constructor arguments, shapes and the noise description, the online
        and target parameters, Adam's ``m``, ``v`` and step count,
        ``num_timesteps``, the generator's state (``replay_t`` included) and
        an Ornstein-Uhlenbeck process's state.  ``memory=True`` adds the valid
        records of the replay memory with ``size`` and ``pos``: after
        ``distribute`` that is this rank's memory only (the parameters and the
        optimiser are every rank's)."""
        opt = self.get_opt_state()
        g = self.rng.state()
        arrays = {'meta': np.array(json.dumps(self._meta())),
                  'params': self.get_parameters(), 'target': self.get_parameters(target=True),
                  'opt_m': opt['m'], 'opt_v': opt['v'], 'opt_step': np.array(opt['step'], np.int64),
                  'num_timesteps': np.array(self.num_timesteps, np.int64),
                  'rng': np.array([g['seed'], g['row_offset'], g['t'], g['epoch'],
                                   g['predict_t'], g['replay_t']], np.uint64)}
        ou = getattr(self.action_noise, 'get_state', lambda: None)()
        if ou is not None:
            arrays['ou_state'], arrays['ou_dones'] = ou
        if memory:
            mem = self.memory
            arrays['mem_size_pos'] = np.array([mem.size, mem.pos], np.int64)
            for name in mem.FIELDS:
                arrays['mem_' + name] = getattr(mem, name)[:mem.size].cpu().numpy()
        np.savez(save_path, **arrays)

    @classmethod
    def load(cls, load_path, env=None, device='auto', **overrides):
        """The model ``save`` wrote (see ``BaseAgent.load`` for ``env`` and
        ``device``).  ``overrides`` replace constructor arguments
        (``action_noise`` among them).  A file saved with ``memory=True``
        restores the replay memory; otherwise the memory starts empty."""
        data, meta, kwargs, env = cls._read(load_path, env, device, overrides)
        if 'action_noise' not in kwargs:
            kwargs['action_noise'] = ddpg.ActionNoise.from_description(meta.get('action_noise'))
        model = cls(meta.get('policy', 'MlpPolicy'), env, **kwargs)     # no kind: a narrow model
        s = model.spec
        if (s.obs_dim, s.act_dim, list(model.hidden)) != (meta['obs_dim'], meta['act_dim'],
                                                          meta['hidden']):
            raise ValueError('the env maps %d -> %d, the saved model %d -> %d (hidden %s)'
                             % (s.obs_dim, s.act_dim, meta['obs_dim'], meta['act_dim'],
                                meta['hidden']))
        model.set_parameters(data['params'], target=data['target'])
        model.set_opt_state({'m': data['opt_m'], 'v': data['opt_v'],
                             'step': int(data['opt_step'])})
        model.num_timesteps = int(data['num_timesteps'])
        g = [int(v) for v in data['rng']]
        model.rng.set_state({'seed': g[0], 'row_offset': g[1], 't': g[2], 'epoch': g[3],
                             'predict_t': g[4], 'replay_t': g[5]})
        model.seed = g[0]
        if 'ou_state' in data and hasattr(model.action_noise, 'set_state') \
                and 'action_noise' not in overrides:
            model.action_noise.set_state(data['ou_state'], data['ou_dones'])
        if 'mem_size_pos' in data:
            import torch
            mem = model.memory
            size, pos = (int(v) for v in data['mem_size_pos'])
            if s.rows != meta['rows'] or size > mem.capacity or size % s.rows or pos % s.rows \
                    or pos >= mem.capacity:
                raise ValueError('the saved replay memory (%d records of %d-row steps) does not '
                                 'fit this model\'s (%d records, %d rows)'
                                 % (size, meta['rows'], mem.capacity, s.rows))
            for name in mem.FIELDS:
                getattr(mem, name)[:size].copy_(torch.from_numpy(data['mem_' + name]))
            mem.size, mem.pos = size, pos
        return model
