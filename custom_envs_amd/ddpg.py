"""The DDPG learner on the device: the actor, the Q critic, their target
networks, the loss gradients, the two Adam steps and the soft update of
stable-baselines 2.x ``DDPG`` over ``ddpg.MlpPolicy`` as HIP kernels
(``ce_ddpg_*``, csrc/ddpg_kernels.h), and a replay memory the engine and the
actor write straight into, so collect -> sample -> step needs no eager torch
and no host round trip.

The settings are the reference's (run_multiagent_exp_single.py:46-47): every
keyword of SB's ``DDPG`` at its default except ``gamma``, ``actor_lr`` and
``critic_lr`` -- ``layers=[64, 64]``, relu, no layer norm, ``tau=0.001``,
``batch_size=128``, ``observation_range=(-5, 5)``, ``reward_scale=1``, no
parameter noise, no normalisation, no pop-art, ``critic_l2_reg=0``,
``clip_norm=None``.

The ``*_numpy`` functions are the executable statement of the semantics (any
dtype, no GPU) and the checkers of the kernels:

    o        = clip(obs, obs_lo, obs_hi)            (both networks, always)
    actor    x = o; x = relu(x W_l + b_l) per hidden l; a = tanh(x W_out + b_out)
    critic   h = relu(o W_0 + b_0); h = concat(h, action)   (hidden units first)
             h = relu(h W_l + b_l) for hidden l >= 1; Q = h W_out + b_out
    act      action = a (+ noise, then clip to [-1, 1], when noise is given)
             env_action = action * scale
    noise    a tensor, or formed inside the act kernel from the counter-based
             generator (``rng.ACTION_NOISE``; ``normal_noise_numpy``,
             ``ou_noise_numpy``): z = N(0,1) of (global row, draw t, column),
             Normal  n  = mean + sigma z
             OU      x' = (x + (theta (mean - x)) dt) + s z,  n = x',
                     s = float32(sigma sqrt(dt)), x = 0 at the start and at
                     the rows whose previous step ended an episode
    sample   the rows of train step t: ``rng.replay_indices_numpy`` (with
             replacement), one draw per step
    target   y = reward + gamma (1 - done1) critic'(obs1, actor'(obs1))
             (' = the target networks; y is a constant of both losses)
    critic   critic_loss = mean((critic(obs0, action) - y)^2)
    actor    actor_loss = -mean(critic(obs0, actor(obs0))), d / d actor only
             (both gradients at the parameters before either update)
    Adam x2  ppo2.adam_step_numpy(max_grad_norm=0, eps=1e-8) with actor_lr on
             the actor's block and critic_lr on the critic's, one shared t
             (baselines' MpiAdam)
    soft     target = (1 - tau) target + tau params, after the Adam steps

Parameters are ONE flat float32 vector ``[actor | critic]`` (``params_layout``);
the targets use the same layout.  The action in the memory and in the critic
is the normalised one in [-1, 1], as SB stores it; SB steps the env with
``action * abs(action_space.low)``, which is ``scale`` here.

``DDPGAgent`` owns the parameters, the targets and Adam's moments on its
device; ``train`` is the train phase of SB's cycle as ONE C call (the indices
of all its steps from one launch, then the steps' launches, no allocation and
no host read), and ``get_opt_state`` / ``set_opt_state`` carry Adam across a
save.  ``agents.DDPG`` is the loop on top (``learn``, ``predict``, ``save``,
``load``).  ``ReplayMemory`` is a device ring of plain torch tensors.  The envs
auto-reset: at a done row ``obs1`` is the reset observation, and ``(1 - done)``
masks it in ``y``.

Limits: 1-2 hidden layers, each 32 or 64 wide (the widths may differ);
``DDPGAgent`` (``ddpg.MlpPolicy``) takes obs_dim <= 128 and act_dim <= 64,
``WideDDPGAgent`` (``ddpg.WideMlpPolicy``) obs_dim <= 1024 and act_dim <= 512
-- the reference's ``Optimize-v0`` is 981 -> 490 -- on tile kernels that walk
the wide layers in chunks (csrc/ddpg_wide_kernels.h) and, at a shape both
take, write the narrow agent's bits.  Anything else raises
``NativeEngineError`` (CE_EUNSUPPORTED); there is no eager fallback.  A wide
agent under a gradient exchange is tested at world 1 only.

Out of scope: parameter noise and layer norm (``LnMlpPolicy``), observation
and return normalisation, pop-art, ``critic_l2_reg``, ``clip_norm``, graph
capture of the loop, a C-side ``[act, env step] x K`` rollout (the collect
loop stays Python-issued), an uneven ``batch_size`` per rank.

Data-parallel training (``distributed.GradientExchange(agent, rank, world)``,
as stable-baselines' MPI workers average gradients through ``MpiAdam``): W
ranks, rank r holding n_r sampled rows of its own memory, take the single
agent's train step on the concatenation, N = sum n_r.  ``partial`` writes the
rank's float64 record (``learner.pack_record_numpy``'s layout: the per
parameter sums of its rows' gradient terms weighted 1 / N, before any
rounding, the statistic sums, n_r), ONE in-place all-gather gives every rank
every record, and ``apply`` adds them in rank order and rounds once
(``combine_records_numpy``), so the replicas stay bit-identical; at W = 1
``partial`` + ``apply`` leave the bits of ``step``.  With an exchange attached
``step`` / ``grad`` / ``train`` do this themselves.
"""
import ctypes
from collections import OrderedDict, namedtuple

import numpy as np

from custom_envs_amd import _native, learner
from custom_envs_amd import rng as _rng
from custom_envs_amd._native import (CeDdpgConfig, CeDdpgNoise, CeDdpgWideConfig, CeDdpgWideNoise,
                                     check)
from custom_envs_amd.learner import N_STATS
from custom_envs_amd.policy import dict_to_flat, flat_to_dict, layout_size
from custom_envs_amd.ppo2 import adam_step_numpy

# the first four of the N_STATS (8) floats a call writes; then two zeros,
# ||critic grad||^2 (at CRITIC_SQ) and ||actor grad||^2 (at ACTOR_SQ)
STAT_NAMES = ('critic_loss', 'actor_loss', 'q_mean', 'target_mean')
CRITIC_SQ, ACTOR_SQ = 6, 7

HyperParams = namedtuple('HyperParams', 'gamma obs_lo obs_hi')
HyperParams.__new__.__defaults__ = (0.99, -5.0, 5.0)

BATCH_FIELDS = ('obs0', 'actions', 'rewards', 'obs1', 'dones')
TARGET_FLAG = 2      # CE_DDPG_TARGET: ce_ddpg_{set,get}_params on the target networks


# ---------------------------------------------------------------------- layout
def params_layout(obs_dim, act_dim, hidden):
    """Ordered name -> (offset, shape) of the flat float32 parameter vector:
    the actor ``actor/w0 [D][h0], actor/b0, ..., actor/w_out [h_last][A],
    actor/b_out``, then the critic ``critic/w0 [D][h0], critic/b0, critic/w1
    [h0 + A][h1], critic/b1, ..., critic/w_out [.][1], critic/b_out``.  The
    ``+ A`` rows (the action, after the hidden units) sit on the layer after
    the first hidden one; with a single hidden layer that is ``w_out``.
    Kernels are row-major ``[in][out]``."""
    layout, off = OrderedDict(), 0

    def add(name, shape):
        nonlocal off
        layout[name] = (off, tuple(shape))
        off += int(np.prod(shape))

    for net, out in (('actor', act_dim), ('critic', 1)):
        width = obs_dim
        for i, h in enumerate(hidden):
            add('%s/w%d' % (net, i), (width, h))
            add('%s/b%d' % (net, i), (h,))
            width = h + act_dim if (net == 'critic' and i == 0) else h
        add('%s/w_out' % net, (width, out))
        add('%s/b_out' % net, (out,))
    return layout


def n_params(obs_dim, act_dim, hidden):
    return layout_size(params_layout(obs_dim, act_dim, hidden))


def n_actor_params(obs_dim, act_dim, hidden):
    """The length of the actor's block (the critic's starts there)."""
    return params_layout(obs_dim, act_dim, hidden)['critic/w0'][0]


def _act_dim_of(n, obs_dim, hidden):
    """A from the flat vector's length (n_params is affine in A)."""
    n0, n1 = n_params(obs_dim, 0, hidden), n_params(obs_dim, 1, hidden)
    act_dim, rest = divmod(n - n0, n1 - n0)
    if rest or act_dim < 1:
        raise ValueError('a flat vector of %d entries fits no act_dim at obs_dim %d, hidden %s'
                         % (n, obs_dim, tuple(hidden)))
    return act_dim


def _as_dict(params, obs_dim, hidden, dtype):
    """The parameter dict in ``dtype`` of a flat vector or a dict, and A."""
    if isinstance(params, dict):
        act_dim = int(np.asarray(params['actor/b_out']).size)
        layout = params_layout(obs_dim, act_dim, hidden)
        if set(params) != set(layout):
            raise ValueError('parameter names differ from the layout: %s'
                             % sorted(set(params) ^ set(layout)))
        return {k: np.asarray(v, dtype) for k, v in params.items()}, act_dim
    flat = np.asarray(params).reshape(-1)
    act_dim = _act_dim_of(flat.size, obs_dim, hidden)
    p = flat_to_dict(flat, params_layout(obs_dim, act_dim, hidden))
    return {k: np.asarray(v, dtype) for k, v in p.items()}, act_dim


def init_params_numpy(obs_dim, act_dim, hidden=(64, 64), seed=0):
    """SB's initialisers as the flat float32 vector: glorot-uniform hidden
    kernels, ``U(-3e-3, 3e-3)`` output kernels, zero biases."""
    rs = np.random.RandomState(seed)
    params = {}
    for name, (_, shape) in params_layout(obs_dim, act_dim, hidden).items():
        if len(shape) == 1:
            value = np.zeros(shape)
        elif name.endswith('w_out'):
            value = rs.uniform(-3e-3, 3e-3, shape)
        else:
            limit = np.sqrt(6.0 / (shape[0] + shape[1]))
            value = rs.uniform(-limit, limit, shape)
        params[name] = value.astype(np.float32)
    return dict_to_flat(params, params_layout(obs_dim, act_dim, hidden))


# ------------------------------------------------------------------ statements
def _clip_obs(obs, obs_range, dtype):
    return np.clip(np.asarray(obs, dtype), dtype(obs_range[0]), dtype(obs_range[1]))


def _actor_forward(p, o, L):
    """(every layer's input, the tanh head's output)."""
    xs = [o]
    for i in range(L):
        xs.append(np.maximum(xs[-1] @ p['actor/w%d' % i] + p['actor/b%d' % i], 0))
    return xs, np.tanh(xs[-1] @ p['actor/w_out'] + p['actor/b_out'])


def _critic_forward(p, o, actions, L):
    """(every layer's input, Q ``[N]``); the action joins layer 1's input
    after the hidden units."""
    xs = [o]
    for i in range(L):
        x = np.maximum(xs[-1] @ p['critic/w%d' % i] + p['critic/b%d' % i], 0)
        xs.append(np.concatenate([x, actions], axis=1) if i == 0 else x)
    return xs, (xs[-1] @ p['critic/w_out'] + p['critic/b_out'])[:, 0]


def _critic_backward(p, xs, dq, grad, dtype):
    """Backprop of ``dq`` (d loss / d Q ``[N]``) through the critic.  With
    ``grad`` a dict the parameter gradients go into it.  Returns d loss / d
    action ``[N][A]``."""
    L = len(xs) - 1
    dz, d_action = dq[:, None], None
    for i in range(L, -1, -1):
        w = 'critic/w_out' if i == L else 'critic/w%d' % i
        b = 'critic/b_out' if i == L else 'critic/b%d' % i
        if grad is not None:
            grad[w] = xs[i].T @ dz
            grad[b] = dz.sum(axis=0)
        if i > 0:
            dx = dz @ p[w].T
            if i == 1:                  # the concat: hidden units, then the action
                h0 = p['critic/w0'].shape[1]
                d_action, dx = dx[:, h0:], dx[:, :h0]
                dz = dx * (xs[1][:, :h0] > 0)
            else:
                dz = dx * (xs[i] > 0)
    return d_action


def actor_numpy(params, obs, noise=None, hidden=(64, 64), obs_range=(-5.0, 5.0),
                dtype=np.float64):
    """The normalised action ``[N][A]`` in [-1, 1] in ``dtype``.  ``params``:
    the flat vector or the ``params_layout`` dict.  With ``noise`` the action
    is ``clip(a + noise, -1, 1)``."""
    obs = np.asarray(obs)
    p, _ = _as_dict(params, obs.shape[1], hidden, dtype)
    _, a = _actor_forward(p, _clip_obs(obs, obs_range, dtype), len(hidden))
    if noise is not None:
        a = np.clip(a + np.asarray(noise, dtype), dtype(-1), dtype(1))
    return a


def critic_numpy(params, obs, actions, hidden=(64, 64), obs_range=(-5.0, 5.0), dtype=np.float64):
    """Q ``[N]`` of the normalised ``actions`` at ``obs`` in ``dtype``."""
    obs = np.asarray(obs)
    p, act_dim = _as_dict(params, obs.shape[1], hidden, dtype)
    actions = np.asarray(actions, dtype).reshape(obs.shape[0], act_dim)
    return _critic_forward(p, _clip_obs(obs, obs_range, dtype), actions, len(hidden))[1]


def target_numpy(target_params, rewards, obs1, dones, gamma=0.99, hidden=(64, 64),
                 obs_range=(-5.0, 5.0), dtype=np.float64):
    """``y = reward + gamma (1 - done1) critic'(obs1, actor'(obs1))`` in
    ``dtype``, ``[N]``.  At a done row ``obs1`` is the reset observation of an
    auto-resetting env; ``(1 - done)`` masks its Q."""
    obs1 = np.asarray(obs1)
    p, _ = _as_dict(target_params, obs1.shape[1], hidden, dtype)
    o = _clip_obs(obs1, obs_range, dtype)
    _, a = _actor_forward(p, o, len(hidden))
    _, q = _critic_forward(p, o, a, len(hidden))
    nonterminal = dtype(1) - (np.asarray(dones) != 0).astype(dtype)
    return np.asarray(rewards, dtype) + dtype(gamma) * nonterminal * q


def loss_grad_numpy(params, target_params, obs0, actions, rewards, obs1, dones,
                    hp=HyperParams(), hidden=(64, 64), dtype=np.float64):
    """Both losses and their gradients in ``dtype`` (manual backprop, NumPy
    only).  Returns (stats dict of STAT_NAMES plus ``critic_sq`` / ``actor_sq``,
    the squared gradient norms; grad in the flat ``params_layout`` order:
    d actor_loss on the actor's block, d critic_loss on the critic's)."""
    obs0 = np.asarray(obs0)
    N, L = obs0.shape[0], len(hidden)
    p, act_dim = _as_dict(params, obs0.shape[1], hidden, dtype)
    layout = params_layout(obs0.shape[1], act_dim, hidden)
    obs_range = (hp[1], hp[2])
    o = _clip_obs(obs0, obs_range, dtype)
    actions = np.asarray(actions, dtype).reshape(N, act_dim)
    y = target_numpy(target_params, rewards, obs1, dones, hp[0], hidden, obs_range, dtype)
    grad = {}

    # the critic's loss at the stored action
    xs, q = _critic_forward(p, o, actions, L)
    err = q - y
    critic_loss = np.mean(err * err)
    _critic_backward(p, xs, dtype(2) * err / dtype(N), grad, dtype)

    # the actor's loss through the critic: d / d actor parameters only
    axs, a = _actor_forward(p, o, L)
    cxs, qa = _critic_forward(p, o, a, L)
    actor_loss = -np.mean(qa)
    d_action = _critic_backward(p, cxs, np.full(N, -1.0 / N, dtype), None, dtype)
    dz = d_action * (dtype(1) - a * a)
    for i in range(L, -1, -1):
        w = 'actor/w_out' if i == L else 'actor/w%d' % i
        b = 'actor/b_out' if i == L else 'actor/b%d' % i
        grad[w] = axs[i].T @ dz
        grad[b] = dz.sum(axis=0)
        if i > 0:
            dz = (dz @ p[w].T) * (axs[i] > 0)

    flat = dict_to_flat(grad, layout, dtype)
    na = layout['critic/w0'][0]
    stats = {'critic_loss': critic_loss, 'actor_loss': actor_loss, 'q_mean': np.mean(q),
             'target_mean': np.mean(y), 'critic_sq': np.sum(flat[na:] * flat[na:]),
             'actor_sq': np.sum(flat[:na] * flat[:na])}
    return stats, flat


def soft_update_numpy(target_params, params, tau=0.001):
    """``(1 - tau) target + tau params`` in the arrays' dtype: two multiplies
    and one add per entry, in this order."""
    target_params, params = np.asarray(target_params), np.asarray(params)
    dt = params.dtype.type
    return dt(1 - tau) * target_params + dt(tau) * params


def train_step_numpy(params, target_params, m, v, t, batch, n_actor, hp=HyperParams(),
                     hidden=(64, 64), tau=0.001, actor_lr=1e-4, critic_lr=1e-3, beta1=0.9,
                     beta2=0.999, eps=1e-8):
    """One DDPG train step in the arrays' dtype: the gradients, Adam on the
    actor's block (the first ``n_actor`` entries) with ``actor_lr`` and on the
    critic's with ``critic_lr`` at the shared 1-based step ``t``, then the soft
    update.  ``batch``: the BATCH_FIELDS dict.  Returns (params,
    target_params, m, v, stats), all new arrays."""
    params, target_params, m, v = (np.asarray(a) for a in (params, target_params, m, v))
    dt = params.dtype.type
    stats, grad = loss_grad_numpy(params, target_params, *[batch[n] for n in BATCH_FIELDS], hp=hp,
                                  hidden=hidden, dtype=dt)
    new = [np.empty_like(params) for _ in range(3)]
    for block, lr in ((slice(0, n_actor), actor_lr), (slice(n_actor, None), critic_lr)):
        out = adam_step_numpy(params[block], grad[block], m[block], v[block], t, lr,
                              max_grad_norm=0, beta1=beta1, beta2=beta2, eps=eps)
        for dst, src in zip(new, out):
            dst[block] = src
    return new[0], soft_update_numpy(target_params, new[0], tau), new[1], new[2], stats


# ---------------------------------------------------- the gradient exchange
# One rank's record is ``learner.pack_record_numpy``'s: ``[n_params sums | 2 *
# ROW_STATS statistic sums | n_r]`` in float64, padded to a multiple of 256 B
# (``learner.record_doubles``); the sums are ``loss_grad_numpy`` of the rank's
# rows weighted ``n_r / N``.
def combine_records_numpy(records, n_params, dtype=np.float64):
    """The statement of ``partial`` + ``combine``: the gradient of all the
    ranks' rows from their records ``[W][>= n_params]``, added in rank order
    in float64, then rounded to ``dtype`` (``learner.combine_records_numpy``
    without an entropy term)."""
    return learner.combine_records_numpy(records, n_params, 0, 0.0, dtype)


# ----------------------------------------------------------------------- noise
class MlpPolicy:
    """The marker stable-baselines scripts pass as DDPG's ``policy``
    (``ddpg.MlpPolicy``): the relu actor and critic of this module."""


class WideMlpPolicy:
    """``ddpg.MlpPolicy`` at wide shapes (obs_dim <= 1024, act_dim <= 512):
    ``agents.DDPG`` builds a ``WideDDPGAgent``."""


POLICY_KINDS = {'MlpPolicy': MlpPolicy, 'WideMlpPolicy': WideMlpPolicy}


def policy_kind(policy):
    """``'MlpPolicy'`` or ``'WideMlpPolicy'`` of a marker class or its name;
    None for anything else."""
    for kind, marker in POLICY_KINDS.items():
        if policy is marker or (isinstance(policy, str) and policy == kind):
            return kind
    return None


def _noise_params(mean, sigma, act_dim):
    """``mean`` and ``sigma`` as float32 ``[A]`` (a scalar broadcasts)."""
    out = []
    for name, value in (('mean', mean), ('sigma', sigma)):
        v = np.asarray(value, np.float32)
        if v.ndim > 1 or (v.ndim == 1 and v.size not in (1, act_dim)):
            raise ValueError('%s must be a scalar or have shape (%d,), got %s'
                             % (name, act_dim, v.shape))
        v = np.array(np.broadcast_to(v.reshape(-1) if v.ndim else v, (act_dim,)))
        if not np.all(np.isfinite(v)):
            raise ValueError('%s must be finite' % name)
        out.append(v)
    if np.any(out[1] < 0):
        raise ValueError('sigma must not be negative')
    return out[0], out[1]


def normal_noise_numpy(mean, sigma, z, dtype=np.float64):
    """``n = mean + sigma * z`` in ``dtype``; ``z [rows][A]`` is
    ``rng.normal_numpy(..., purpose=rng.ACTION_NOISE)``.  ``mean`` / ``sigma``
    are the float32 values the kernel holds (a scalar broadcasts to ``[A]``)."""
    z = np.asarray(z, dtype)
    mean, sigma = _noise_params(mean, sigma, z.shape[-1])
    return mean.astype(dtype) + sigma.astype(dtype) * z


def ou_scale_numpy(sigma, dt):
    """``s = float32(sigma * sqrt(dt))``, formed in double from the float32
    ``sigma``."""
    return (np.asarray(sigma, np.float32).astype(np.float64) * np.sqrt(np.float64(dt))).astype(
        np.float32)


def ou_noise_numpy(x, mean, sigma, z, theta=0.15, dt=1e-2, reset=None, dtype=np.float64):
    """One Ornstein-Uhlenbeck step in ``dtype``: ``x' = (x + (theta * (mean -
    x)) * dt) + s * z`` with ``s = ou_scale_numpy(sigma, dt)``, where ``x
    [rows][A]`` reads as 0 at the rows with ``reset [rows]`` non-zero.  The
    noise is ``x'``, which is also the next state."""
    z = np.asarray(z, dtype)
    mean, sigma = _noise_params(mean, sigma, z.shape[-1])
    x = np.asarray(x, dtype)
    if reset is not None:
        x = np.where((np.asarray(reset) != 0)[:, None], dtype(0), x)
    s = ou_scale_numpy(sigma, dt).astype(dtype)
    return (x + (dtype(theta) * (mean.astype(dtype) - x)) * dtype(dt)) + s * z


class ActionNoise:
    """What ``DDPGAgent.act`` forms inside its kernel when it is passed
    ``noise=(action_noise, device_rng)``; see the module docstring."""
    KIND = None
    theta, dt = 0.0, 0.0

    def __init__(self, mean, sigma):
        self.mean, self.sigma = np.asarray(mean, np.float32), np.asarray(sigma, np.float32)
        _noise_params(self.mean, self.sigma, max(self.mean.size, self.sigma.size))
        self._struct = None

    def params(self, act_dim):
        return _noise_params(self.mean, self.sigma, act_dim)

    def struct(self, act_dim, wide=False):
        """The ``ce_ddpg_noise`` (``wide``: the ``ce_ddpg_wide_noise``) of this
        object at ``act_dim`` (built once)."""
        if self._struct is None or self._struct[0] != (act_dim, wide):
            mean, sigma = self.params(act_dim)
            c = (CeDdpgWideNoise if wide else CeDdpgNoise)(
                kind=self.KIND, theta=float(self.theta), dt=float(self.dt))
            if act_dim > len(c.mean):
                raise ValueError('the noise description holds %d columns, act_dim is %d'
                                 % (len(c.mean), act_dim))
            for i in range(act_dim):
                c.mean[i], c.sigma[i] = float(mean[i]), float(sigma[i])
            self._struct = ((act_dim, wide), c)
        return self._struct[1]

    def reset(self):
        pass

    def describe(self):
        """JSON-able constructor arguments (``from_description`` inverts)."""
        d = {'kind': type(self).__name__, 'mean': [float(v) for v in self.mean.reshape(-1)],
             'sigma': [float(v) for v in self.sigma.reshape(-1)]}
        if self.KIND == _native.CE_DDPG_NOISE_OU:
            d.update(theta=float(self.theta), dt=float(self.dt))
        return d

    @staticmethod
    def from_description(d):
        if d is None:
            return None
        mean, sigma = np.asarray(d['mean'], np.float32), np.asarray(d['sigma'], np.float32)
        if d['kind'] == 'NormalActionNoise':
            return NormalActionNoise(mean, sigma)
        if d['kind'] == 'OrnsteinUhlenbeckActionNoise':
            return OrnsteinUhlenbeckActionNoise(mean, sigma, theta=d['theta'], dt=d['dt'])
        raise ValueError('unknown action noise %r' % (d['kind'],))


class NormalActionNoise(ActionNoise):
    """stable-baselines' ``NormalActionNoise(mean, sigma)``, per column."""
    KIND = _native.CE_DDPG_NOISE_NORMAL

    def noise_numpy(self, z, dtype=np.float64):
        return normal_noise_numpy(self.mean, self.sigma, z, dtype)


class OrnsteinUhlenbeckActionNoise(ActionNoise):
    """stable-baselines' ``OrnsteinUhlenbeckActionNoise(mean, sigma, theta,
    dt)`` with ``initial_noise=None``.  The object owns the process state ``x
    [rows][A]`` (``state``, a device tensor made at the first use) and the
    last step's ``dones`` (``last_dones``), which restart the rows whose
    episode ended (SB's ``action_noise.reset()``)."""
    KIND = _native.CE_DDPG_NOISE_OU

    def __init__(self, mean, sigma, theta=0.15, dt=1e-2):
        super().__init__(mean, sigma)
        self.theta, self.dt = float(theta), float(dt)
        if not np.isfinite(self.theta) or not self.dt > 0 or not np.isfinite(self.dt):
            raise ValueError('theta must be finite and dt positive')
        self.state = self.last_dones = None
        self._pending = None         # a loaded host state, until a device is known

    def step_numpy(self, x, z, reset=None, dtype=np.float64):
        return ou_noise_numpy(x, self.mean, self.sigma, z, self.theta, self.dt, reset, dtype)

    def ensure_state(self, rows, act_dim, device):
        """``state`` and ``last_dones`` as tensors on ``device`` (a torch
        device), zero at the first use."""
        import torch
        if self.state is None or tuple(self.state.shape) != (rows, act_dim) \
                or self.state.device != device:
            self.state = torch.zeros((rows, act_dim), dtype=torch.float32, device=device)
            self.last_dones = torch.zeros(rows, dtype=torch.uint8, device=device)
            if self._pending is not None:
                x, d = self._pending
                if x.shape == (rows, act_dim):
                    self.state.copy_(torch.from_numpy(x))
                    self.last_dones.copy_(torch.from_numpy(d))
                self._pending = None
        return self.state

    def reset(self):
        if self.state is not None:
            self.state.zero_()
            self.last_dones.zero_()
        self._pending = None

    def get_state(self):
        """(x ``[rows][A]`` float32, dones ``[rows]`` uint8) as numpy, or
        None before the first use."""
        if self.state is None:
            return self._pending
        return self.state.cpu().numpy(), self.last_dones.cpu().numpy()

    def set_state(self, x, dones):
        x = np.ascontiguousarray(x, np.float32)
        dones = np.ascontiguousarray(dones, np.uint8)
        if x.ndim != 2 or dones.shape != (x.shape[0],):
            raise ValueError('OU state must be [rows][A] with dones [rows]')
        self.state = self.last_dones = None
        self._pending = (x, dones)


def check_generated_noise(noise, rows=None, act_dim=None, wide=False):
    """``noise=(action_noise, device_rng)``: the pair's form.  Returns it."""
    if not isinstance(noise, tuple) or len(noise) != 2 \
            or not isinstance(noise[0], ActionNoise) or not isinstance(noise[1], _rng.DeviceRng):
        raise ValueError('noise must be a float32 tensor, None or (ActionNoise, DeviceRng), got %r'
                         % (noise,))
    if act_dim is not None:
        noise[0].struct(act_dim, wide)   # validates the columns once, then cached
    if rows is not None and noise[1].row_offset + rows > 2 ** 32:
        raise ValueError('rows row_offset .. row_offset + rows - 1 must stay below 2^32')
    return noise


# ----------------------------------------------------------------------- agent
class Stats(learner.Stats):
    """The statistics of one ``grad`` / ``step`` call as a device tensor
    (``.tensor``: STAT_NAMES, two zeros, ||critic grad||^2, ||actor grad||^2);
    ``.stats()`` copies them out.  ``.y``: the targets ``[N]`` of the call's
    rows, the device tensor the call computed them into."""
    names = STAT_NAMES

    def __init__(self, tensor, y=None):
        super().__init__(tensor)
        self.y = y

    def stats(self):
        host = self.tensor.detach().cpu().numpy()
        out = {name: float(host[i]) for i, name in enumerate(self.names)}
        out['critic_grad_norm'] = float(np.sqrt(host[CRITIC_SQ]))
        out['actor_grad_norm'] = float(np.sqrt(host[ACTOR_SQ]))
        return out


def check_tensor(name, t, dtype, shape):
    """dtype, shape, contiguity (``policy.check_input``'s order; the device
    comes last, with the caller)."""
    if not hasattr(t, 'data_ptr'):
        raise ValueError('%s must be a torch tensor, got %s' % (name, type(t).__name__))
    if t.dtype != dtype:
        raise ValueError('%s must have dtype %s, got %s'
                         % (name, str(dtype).replace('torch.', ''), t.dtype))
    if tuple(t.shape) != tuple(shape):
        raise ValueError('%s must have shape %s, got %s' % (name, tuple(shape), tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError('%s must be contiguous' % name)


class DDPGAgent(learner.LearnerBase):
    """DDPG's actor, critic, targets and optimiser on one GPU (see the module
    docstring), on the learners' shared shell (``learner.LearnerBase``); its
    own are the shape-only store, the targets, ``Stats.y``, ``stats=`` in
    ``apply`` and the two learning rates.  ``device=None`` gives the
    shape-and-validation-only form, which needs no GPU.  ``scale`` (``[A]`` or a scalar): what the normalised
    action is multiplied by for the env, SB's ``abs(action_space.low)``.
    ``grid_limit`` 0 means one workgroup per CU per branch."""
    PREFIX = 'ce_ddpg'
    BATCH_FIELDS = BATCH_FIELDS
    STATS = Stats
    MAX_OBS, MAX_ACT = 128, _native.CE_DDPG_MAX_ACT
    WIDE = False                 # the wide create entry, config and noise structs

    def __init__(self, obs_dim, act_dim, hidden=(64, 64), scale=1.0, gamma=0.99, tau=0.001,
                 actor_lr=1e-4, critic_lr=1e-3, obs_range=(-5.0, 5.0), beta1=0.9, beta2=0.999,
                 eps=1e-8, grid_limit=0, device=0):
        lib = _native.load()
        self.obs_dim, self.act_dim = int(obs_dim), int(act_dim)
        self.hidden = tuple(int(h) for h in hidden)
        self.device = 0 if device is None else int(device)
        if not 1 <= len(self.hidden) <= 2:
            raise _native.NativeEngineError('the DDPG networks take 1 or 2 hidden layers')
        if not 1 <= self.act_dim <= self.MAX_ACT:
            raise _native.NativeEngineError('act_dim must be in [1, %d], got %d'
                                            % (self.MAX_ACT, self.act_dim))
        self.gamma, self.tau = float(gamma), float(tau)
        self.actor_lr, self.critic_lr = float(actor_lr), float(critic_lr)
        self.obs_range = (float(obs_range[0]), float(obs_range[1]))
        self.hp = HyperParams(self.gamma, *self.obs_range)
        self.scale = np.ascontiguousarray(
            np.broadcast_to(np.asarray(scale, np.float32), (self.act_dim,)))
        suffix = '_wide' if self.WIDE else ''
        self._cfg = cfg = (CeDdpgWideConfig if self.WIDE else CeDdpgConfig)(
            abi_version=_native.ABI_VERSION, device=self.device, obs_dim=self.obs_dim,
            act_dim=self.act_dim, n_hidden=len(self.hidden), grid_limit=int(grid_limit),
            gamma=self.gamma, tau=self.tau, actor_lr=self.actor_lr, critic_lr=self.critic_lr,
            beta1=float(beta1), beta2=float(beta2), eps=float(eps), obs_lo=self.obs_range[0],
            obs_hi=self.obs_range[1])
        for i, h in enumerate(self.hidden):
            cfg.hidden[i] = h
        for i, s in enumerate(self.scale):
            cfg.scale[i] = float(s)
        n = getattr(lib, 'ce_ddpg_n_params' + suffix)(ctypes.byref(cfg))
        if n < 0:
            check(n, 'ce_ddpg_n_params' + suffix)
        self.n_params = int(n)
        self.n_actor = n_actor_params(self.obs_dim, self.act_dim, self.hidden)
        self._lib, self._h = lib, None
        self._host_params = self._host_target = None
        self._host_opt = None
        self._train_scratch = None
        if device is None:      # shape only: layout, statements and validation, no GPU
            self._host_opt = {'m': np.zeros(self.n_params, np.float32),
                              'v': np.zeros(self.n_params, np.float32), 'step': 0}
            return
        handle = ctypes.c_void_p()
        check(getattr(lib, 'ce_ddpg_create' + suffix)(ctypes.byref(cfg), ctypes.byref(handle)),
              'ce_ddpg_create' + suffix)
        self._h = handle

    def params_layout(self):
        return params_layout(self.obs_dim, self.act_dim, self.hidden)

    def _need_handle(self):
        if self._h is None:
            raise _native.NativeEngineError('a shape-only agent has no device')

    # -------------------------------------------------------------- parameters
    def set_params(self, params, stream=None, target_only=False):
        """The online parameters (flat vector or ``params_layout`` dict, numpy
        or a float32 device tensor), copied into the targets too (SB's
        initialisation: the soft update with tau = 1).  Adam's moments and
        step count are kept.  ``target_only``: the targets alone (a saved
        model's, after its online parameters)."""
        if isinstance(params, dict):
            params = dict_to_flat(params, self.params_layout())
        flags = TARGET_FLAG if target_only else 0
        if hasattr(params, 'data_ptr'):
            import torch
            check_tensor('params', params, torch.float32, (self.n_params,))
            if self._h is None:
                raise ValueError('a shape-only agent takes host parameters')
            self.check_device('params', params)
            self._call('set_params', self._h, params.data_ptr(), self.n_params,
                       flags | _native.CE_PTR_DEVICE, self._stream(stream))
            self._host_params = self._host_target = None
            return
        flat = np.ascontiguousarray(params, dtype=np.float32).reshape(-1)
        if flat.size != self.n_params:
            raise ValueError('got %d parameters, the agent has %d' % (flat.size, self.n_params))
        if self._h is not None:
            self._call('set_params', self._h, flat.ctypes.data, flat.size, flags,
                       self._stream(stream))
        self._host_target = flat.copy()
        if not target_only:
            self._host_params = flat.copy()

    def get_params(self, target=False, out=None, stream=None):
        """The online (``target``: the target) parameters: into the float32
        device tensor ``out`` (stream-ordered), or as a new numpy vector
        (synchronises).  The shape-only agent returns what was set."""
        if self._h is None:
            host = self._host_target if target else self._host_params
            if host is None:
                raise ValueError('no parameters were set')
            return host.copy()
        flags = TARGET_FLAG if target else 0
        if out is not None:
            import torch
            check_tensor('out', out, torch.float32, (self.n_params,))
            self.check_device('out', out)
            self._call('get_params', self._h, out.data_ptr(), self.n_params,
                       flags | _native.CE_PTR_DEVICE, self._stream(stream))
            return out
        flat = np.empty(self.n_params, np.float32)
        self._call('get_params', self._h, flat.ctypes.data, flat.size, flags, self._stream(stream))
        return flat

    # --------------------------------------------------------- optimiser state
    OPT_BLOCKS = ('m', 'v')

    # get_opt_state / set_opt_state differ from the base's for the shape-only
    # agent alone, which keeps what was set on the host (zeros at first)
    def get_opt_state(self, stream=None):
        """Adam's state as a dict: ``m`` and ``v`` (new float32 numpy vectors
        in the flat layout) and ``step``, the shared step count.
        Synchronises.  The shape-only agent returns what was set (zeros)."""
        if self._h is None:
            return {k: (v.copy() if hasattr(v, 'copy') else v) for k, v in self._host_opt.items()}
        return super().get_opt_state(stream)

    def set_opt_state(self, state, stream=None):
        """Install a ``get_opt_state`` dict (validated first).  The
        parameters and the targets are kept."""
        if self._h is not None:
            return super().set_opt_state(state, stream)
        m, v, step = self.check_opt_state(state)
        self._host_opt = {'m': m.copy(), 'v': v.copy(), 'step': step}

    # --------------------------------------------------------------------- act
    def check_act(self, obs, noise=None, out=None):
        """The form of ``act``'s tensors, then where each lives.  Returns the
        row count."""
        import torch
        rows = int(obs.shape[0]) if hasattr(obs, 'dim') and obs.dim() == 2 else -1
        check_tensor('obs', obs, torch.float32, (max(rows, 1), self.obs_dim))
        generated = isinstance(noise, tuple)
        if generated:
            check_generated_noise(noise, max(rows, 1), self.act_dim, self.WIDE)
        elif noise is not None:
            check_tensor('noise', noise, torch.float32, (rows, self.act_dim))
        if out is not None:
            for name in ('action', 'env_action'):
                if out.get(name) is None:
                    raise ValueError('act outputs lack %r' % name)
                check_tensor('act output ' + name, out[name], torch.float32, (rows, self.act_dim))
        if self._h is None:
            return rows
        self.check_device('obs', obs)
        if noise is not None and not generated:
            self.check_device('noise', noise)
        if out is not None:
            for name in ('action', 'env_action'):
                self.check_device('act output ' + name, out[name])
        return rows

    def act(self, obs, noise=None, out=None, stream=None, t=None, reset=None):
        """One stream-ordered launch over ``obs [rows][D]`` for any row count
        (``noise [rows][A]`` or None: the caller's Normal or
        Ornstein-Uhlenbeck draw).  Returns ``out`` (allocated when None):
        ``action`` (normalised, what the memory stores) and ``env_action``
        (``action * scale``, what the env reads).

        ``noise=(action_noise, device_rng)``: the kernel forms the noise
        itself at draw ``t`` (default ``device_rng.t``; the generator is not
        advanced) for the global rows ``device_rng.row_offset + r``.  An
        Ornstein-Uhlenbeck object's state is read and written in place;
        ``reset`` (uint8 ``[rows]`` device tensor or None) marks the rows
        whose state reads as 0, the previous step's ``dones``."""
        import torch
        rows = self.check_act(obs, noise, out)
        if isinstance(noise, tuple):
            return self._act_generated(obs, rows, noise, out, stream, t, reset)
        if out is None:
            out = {n: torch.empty((rows, self.act_dim), dtype=torch.float32, device=obs.device)
                   for n in ('action', 'env_action')}
        self._call('act', self._h, obs.data_ptr(), None if noise is None else noise.data_ptr(),
                   rows, out['action'].data_ptr(), out['env_action'].data_ptr(),
                   self._stream(stream))
        return out

    def _act_generated(self, obs, rows, noise, out, stream, t, reset):
        import torch
        action_noise, gen = noise
        t = int(gen.t) if t is None else int(t)
        if not 0 <= t < 2 ** 32:
            raise ValueError('the draw t must be in [0, 2^32), got %d' % t)
        self._need_handle()
        state_ptr = reset_ptr = None
        if action_noise.KIND == _native.CE_DDPG_NOISE_OU:
            state_ptr = action_noise.ensure_state(rows, self.act_dim, obs.device).data_ptr()
            if reset is not None:
                check_tensor('reset', reset, torch.uint8, (rows,))
                self.check_device('reset', reset)
                reset_ptr = reset.data_ptr()
        if out is None:
            out = {n: torch.empty((rows, self.act_dim), dtype=torch.float32, device=obs.device)
                   for n in ('action', 'env_action')}
        self._call('act_rng_wide' if self.WIDE else 'act_rng', self._h, obs.data_ptr(), rows,
                   gen.seed, t, gen.row_offset,
                   ctypes.byref(action_noise.struct(self.act_dim, self.WIDE)), state_ptr, reset_ptr,
                   out['action'].data_ptr(), out['env_action'].data_ptr(), self._stream(stream))
        return out

    # ------------------------------------------------------------------- batch
    def check_batch(self, batch, idx=None):
        """The form of a batch (``obs0`` / ``obs1 [M][D]``, ``actions [M][A]``,
        ``rewards [M]`` float32, ``dones [M]`` uint8, contiguous) and of
        ``idx`` (int32 ``[N]``), then where each lives.  Returns (M, N)."""
        import torch
        for name in BATCH_FIELDS:
            if batch.get(name) is None:
                raise ValueError('batch lacks %r' % name)
        obs = batch['obs0']
        if not hasattr(obs, 'dim') or obs.dim() != 2:
            raise ValueError('obs0 must have shape [M][%d], got %s'
                             % (self.obs_dim, tuple(getattr(obs, 'shape', ()))))
        M = int(obs.shape[0])
        if M < 1:
            raise ValueError('obs0 must hold at least one row')
        shapes = {'obs0': (M, self.obs_dim), 'obs1': (M, self.obs_dim),
                  'actions': (M, self.act_dim)}
        for name in BATCH_FIELDS:
            check_tensor(name, batch[name], torch.uint8 if name == 'dones' else torch.float32,
                         shapes.get(name, (M,)))
        N = M if idx is None else self.check_idx(idx)
        if self._h is not None:
            for name in BATCH_FIELDS:
                self.check_device(name, batch[name])
            if idx is not None:
                self.check_device('idx', idx)
        return M, N

    def _head(self, batch, idx):
        M, N = self.check_batch(batch, idx)
        self._need_handle()
        ptrs = [batch[n].data_ptr() for n in BATCH_FIELDS]
        return [self._h, N, M, None if idx is None else idx.data_ptr()] + ptrs, N

    def target(self, batch, idx=None, stream=None):
        """``y [N]`` of the rows ``idx`` (None: all) of ``batch``, a float32
        device tensor."""
        import torch
        head, N = self._head(batch, idx)
        y = torch.empty(N, dtype=torch.float32, device=batch['obs0'].device)
        h, n, m, ix, _, _, rewards, obs1, dones = head
        self._call('target', h, n, m, ix, obs1, rewards, dones, y.data_ptr(), self._stream(stream))
        return y

    def grad(self, batch, idx=None, stream=None):
        """Both loss gradients of the rows ``idx`` (None: all) of ``batch``,
        no update.  Returns (grad ``[n_params]`` device tensor, ``Stats``)."""
        import torch
        if self.exchange is not None:      # the gradient of every rank's rows
            records, n_total, y = self._exchange_records(batch, idx, stream)
            grad, stats = self.combine(records, n_total, stream=stream)
            stats.y = y
            return grad, stats
        head, N = self._head(batch, idx)
        dev = batch['obs0'].device
        grad = torch.empty(self.n_params, dtype=torch.float32, device=dev)
        y = torch.empty(N, dtype=torch.float32, device=dev)
        stats = torch.empty(N_STATS, dtype=torch.float32, device=dev)
        self._call('grad', *head, y.data_ptr(), grad.data_ptr(), stats.data_ptr(),
                   self._stream(stream))
        return grad, Stats(stats, y=y)

    # ------------------------------------------------------- gradient exchange
    # W ranks, rank r holding n_r sampled rows, take the single agent's train
    # step on the concatenation, N = sum n_r: ``partial`` (target, gradient
    # with 1 / N, this rank's float64 record), the caller's all-gather of the
    # ``[W][record]`` buffer, ``apply`` (combine in rank order, statistics,
    # Adam x2 + soft update).  Every rank computes the same bits; at W = 1 they
    # are ``step``'s.
    def check_record_tensor(self, name, t, shape):
        """The base's check with ``check_tensor``'s texts, as every other
        tensor of this module is refused."""
        import torch
        check_tensor(name, t, torch.float64, shape)
        if self._h is not None:
            self.check_device(name, t)

    def partial(self, batch, idx=None, n_total=None, out=None, stream=None, y=None):
        """This rank's share of a train step of ``n_total`` rows (None: its
        own ``n``): the targets and both loss gradients of the rows ``idx``
        with the row weight ``1 / n_total``, as one float64 record in ``out``
        (``[record_doubles]``; None: a new tensor).  ``y`` (float32 ``[N]``
        or None: a new tensor) receives the rows' targets.  Returns the
        record."""
        return self._partial(batch, idx, n_total, out, y, stream)[0]

    def _partial(self, batch, idx, n_total, out, y, stream):
        """``partial``: (the record, y)."""
        import torch
        n_total = self.check_total(self._rows_of(batch, idx), n_total)
        if out is not None:
            self.check_record_tensor('out', out, (self.record_doubles,))
        M, N = self.check_batch(batch, idx)
        if y is not None:
            check_tensor('y', y, torch.float32, (N,))
        self._need_handle()
        dev = batch['obs0'].device
        if y is None:
            y = torch.empty(N, dtype=torch.float32, device=dev)
        else:
            self.check_device('y', y)
        if out is None:
            out = torch.zeros(self.record_doubles, dtype=torch.float64, device=dev)
        self._call('partial', self._h, N, n_total, M, None if idx is None else idx.data_ptr(),
                   *[batch[n].data_ptr() for n in BATCH_FIELDS], y.data_ptr(), out.data_ptr(),
                   self._stream(stream))
        return out, y

    def _records_head(self, records, n_total, stats=None):
        """The base's, except that a shape-only agent is refused here and
        that ``apply``'s ``stats`` (checked) is written instead of a new
        tensor."""
        import torch
        world, n_total = self.check_gathered(records, n_total)
        self._need_handle()
        if stats is None:
            stats = torch.empty(N_STATS, dtype=torch.float32, device=records.device)
        else:
            check_tensor('stats', stats, torch.float32, (N_STATS,))
            self.check_device('stats', stats)
        return [self._h, world, records.data_ptr(), n_total], stats

    def apply(self, records, n_total, actor_lr=None, critic_lr=None, stream=None, stats=None):
        """Combine, statistics, then ``step``'s update (Adam on both blocks,
        one step; the soft update; both images) from the ranks' records.
        ``stats``: the float32 ``[8]`` device tensor to write (None: a new
        one).  Returns ``Stats``."""
        actor_lr, critic_lr = self._rate('actor_lr', actor_lr), self._rate('critic_lr', critic_lr)
        head, stats = self._records_head(records, n_total, stats)
        self._call('apply', *head, actor_lr, critic_lr, stats.data_ptr(), self._stream(stream))
        self._host_params = self._host_target = None
        return Stats(stats)

    def _exchange_records(self, batch, idx, stream, y=None):
        """partial, the gather: (the gathered records, n_total, y)."""
        ex = self.exchange
        n_total = ex.total_rows(self._rows_of(batch, idx))
        _, y = self._partial(batch, idx, n_total, ex.records[ex.rank], y, stream)
        return ex.gather_records(), n_total, y

    @staticmethod
    def _rate(name, value):
        """A per-call learning rate for C: None is -1 (the agent's own), zero
        freezes that block for the call, a negative or NaN rate is refused."""
        if value is None:
            return -1.0
        value = float(value)
        if not value >= 0.0:
            raise ValueError('%s must be >= 0 (0 leaves that network where it is), got %r'
                             % (name, value))
        return value

    def step(self, batch, idx=None, actor_lr=None, critic_lr=None, stream=None):
        """One train step as one stream-ordered call of five launches: target,
        gradient, reduce, statistics, and Adam x2 + soft update + the images'
        repack.  ``actor_lr`` / ``critic_lr`` override the agent's for this
        call; 0 leaves that network's parameters where they are (Adam's
        moments and the soft update still move).  Returns ``Stats``.  With a
        gradient exchange attached it is the step on every rank's rows:
        partial, one in-place all-gather, apply."""
        import torch
        if self.exchange is not None:
            self._rate('actor_lr', actor_lr), self._rate('critic_lr', critic_lr)
            records, n_total, y = self._exchange_records(batch, idx, stream)
            stats = self.apply(records, n_total, actor_lr, critic_lr, stream=stream)
            stats.y = y
            return stats
        actor_lr, critic_lr = self._rate('actor_lr', actor_lr), self._rate('critic_lr', critic_lr)
        head, N = self._head(batch, idx)
        dev = batch['obs0'].device
        y = torch.empty(N, dtype=torch.float32, device=dev)
        stats = torch.empty(N_STATS, dtype=torch.float32, device=dev)
        self._call('step', *head, y.data_ptr(), actor_lr, critic_lr, stats.data_ptr(),
                   self._stream(stream))
        self._host_params = self._host_target = None
        return Stats(stats, y=y)

    def check_train(self, memory, steps, batch_size, rng):
        """The form of ``train``'s arguments (no GPU).  Returns (steps, n)."""
        if not isinstance(memory, ReplayMemory):
            raise TypeError('memory must be a ReplayMemory')
        if not isinstance(rng, _rng.DeviceRng):
            raise TypeError('rng must be a DeviceRng')
        if (memory.obs_dim, memory.act_dim) != (self.obs_dim, self.act_dim):
            raise ValueError('the memory holds obs_dim %d, act_dim %d, the agent maps %d -> %d'
                             % (memory.obs_dim, memory.act_dim, self.obs_dim, self.act_dim))
        if memory.size < 1:
            raise ValueError('the memory is empty')
        steps, n, _ = rng.check_replay(steps, batch_size, memory.size)
        return steps, n

    def train(self, memory, steps, batch_size, rng, actor_lr=None, critic_lr=None, stream=None):
        """The train phase as ONE stream-ordered C call: one launch draws the
        ``[steps][batch_size]`` replay indices (``rng.replay_indices`` of the
        draws ``rng.replay_t ..`` over the memory's ``size`` valid records),
        then ``steps`` x the five launches of ``step``.  No allocation beyond
        the returned statistics (the index and target buffers are kept across
        calls) and no host read; bit-equal to ``steps`` calls of
        ``step(memory.as_batch(), idx[s])``.  Advances ``rng.replay_t`` and
        Adam's count by ``steps``.  Returns the ``[steps][8]`` statistics, a
        device tensor; ``Stats(result[-1])`` names its last row.

        With a gradient exchange attached a gather sits between a step's two
        halves, so the call is one launch for the indices, then ``steps`` x
        (partial, all-gather, apply) issued from here on one stream.  A step's
        index stream has ``world * batch_size`` words; rank r maps the columns
        ``[r * batch_size, (r + 1) * batch_size)`` onto its own memory's
        ``size`` (``rng.replay_indices_numpy(..., offset, total)``), and the
        step is the single agent's on the ``world * batch_size`` rows."""
        import torch
        if self.exchange is not None:
            return self._train_exchange(memory, steps, batch_size, rng, actor_lr, critic_lr,
                                        stream)
        actor_lr, critic_lr = self._rate('actor_lr', actor_lr), self._rate('critic_lr', critic_lr)
        steps, n = self.check_train(memory, steps, batch_size, rng)
        self._need_handle()
        self.check_device('memory', memory.obs0)
        dev = memory.obs0.device
        sc = self._train_scratch
        if sc is None or sc['idx'].shape != (steps, n) or sc['idx'].device != dev:
            sc = self._train_scratch = {
                'idx': torch.empty((steps, n), dtype=torch.int32, device=dev),
                'y': torch.empty(n, dtype=torch.float32, device=dev)}
        stats = torch.empty((steps, N_STATS), dtype=torch.float32, device=dev)
        self._call('train', self._h, steps, n, memory.size, rng.seed, int(rng.replay_t),
                   *[getattr(memory, f).data_ptr() for f in BATCH_FIELDS], sc['idx'].data_ptr(),
                   sc['y'].data_ptr(), actor_lr, critic_lr, stats.data_ptr(),
                   self._stream(stream))
        rng.advance_replay(steps)
        self._host_params = self._host_target = None
        return stats

    def _train_exchange(self, memory, steps, batch_size, rng, actor_lr, critic_lr, stream):
        """``train`` under a gradient exchange (see there)."""
        import torch
        ex = self.exchange
        self._rate('actor_lr', actor_lr), self._rate('critic_lr', critic_lr)
        steps, n = self.check_train(memory, steps, batch_size, rng)
        total = ex.world * n
        rng.check_replay(steps, total, memory.size)
        self._need_handle()
        self.check_device('memory', memory.obs0)
        dev = memory.obs0.device
        sc = self._train_scratch
        if sc is None or sc['idx'].shape != (steps, total) or sc['idx'].device != dev:
            sc = self._train_scratch = {
                'idx': torch.empty((steps, total), dtype=torch.int32, device=dev),
                'y': torch.empty(n, dtype=torch.float32, device=dev)}
        stats = torch.empty((steps, N_STATS), dtype=torch.float32, device=dev)
        idx = rng.replay_indices(steps, n, memory.size, stream=stream, offset=ex.rank * n,
                                 total=total, out=sc['idx'])
        batch, record = memory.as_batch(), ex.records[ex.rank]
        for s in range(steps):
            self._partial(batch, idx[s], total, record, sc['y'], stream)
            self.apply(ex.gather_records(), total, actor_lr, critic_lr, stream=stream,
                       stats=stats[s])
        rng.advance_replay(steps)
        return stats

    def loss_grad_numpy(self, params, target_params, batch, dtype=np.float64):
        """``loss_grad_numpy`` with this agent's shape and hyper-parameters."""
        return loss_grad_numpy(params, target_params, *[batch[n] for n in BATCH_FIELDS],
                               hp=self.hp, hidden=self.hidden, dtype=dtype)


class WideDDPGAgent(DDPGAgent):
    """``DDPGAgent`` at obs_dim <= 1024 and act_dim <= 512, through
    ``ce_ddpg_create_wide``: the act, target and gradient kernels walk the wide
    layers in chunks (csrc/ddpg_wide_kernels.h); every other entry and kernel
    is the narrow agent's.  ``grid_limit`` 0 means at most 64 workgroups per
    branch (a gradient partial is about 0.8 MB at 981 -> 490)."""
    MAX_OBS, MAX_ACT = _native.CE_DDPG_WIDE_MAX_OBS, _native.CE_DDPG_WIDE_MAX_ACT
    WIDE = True


AGENTS = {'MlpPolicy': DDPGAgent, 'WideMlpPolicy': WideDDPGAgent}


# ---------------------------------------------------------------------- memory
class ReplayMemory:
    """A device ring of ``capacity`` transitions as plain torch tensors:
    ``obs0 [C][D]``, ``actions [C][A]``, ``rewards [C]``, ``obs1 [C][D]``
    (float32) and ``dones [C]`` (uint8).  One env step appends ``rows``
    records as ONE contiguous slice of every field (``slot()``), so the engine
    and the actor write straight into it; ``capacity`` must be a multiple of
    ``rows``.  ``device=None`` keeps the tensors on the host (the argument
    checks need no GPU)."""
    FIELDS = BATCH_FIELDS

    def __init__(self, capacity, rows, obs_dim, act_dim, device=0):
        import torch
        self.capacity, self.rows = int(capacity), int(rows)
        self.obs_dim, self.act_dim = int(obs_dim), int(act_dim)
        if self.rows < 1:
            raise ValueError('rows must be >= 1, got %d' % self.rows)
        if self.capacity < self.rows or self.capacity % self.rows:
            raise ValueError('capacity (%d) must be a positive multiple of rows (%d)'
                             % (self.capacity, self.rows))
        self.device = device
        dev = torch.device('cpu') if device is None else torch.device('cuda', int(device))
        C, f32 = self.capacity, torch.float32
        self.obs0 = torch.zeros((C, self.obs_dim), dtype=f32, device=dev)
        self.actions = torch.zeros((C, self.act_dim), dtype=f32, device=dev)
        self.rewards = torch.zeros(C, dtype=f32, device=dev)
        self.obs1 = torch.zeros((C, self.obs_dim), dtype=f32, device=dev)
        self.dones = torch.zeros(C, dtype=torch.uint8, device=dev)
        self.size = 0        # valid records
        self.pos = 0         # where the next step's records go

    def slot(self):
        """The slice of every field the next env step writes."""
        return slice(self.pos, self.pos + self.rows)

    def advance(self):
        """One env step's records were written at ``slot()``."""
        self.pos = (self.pos + self.rows) % self.capacity
        self.size = min(self.size + self.rows, self.capacity)

    def as_batch(self):
        """The whole ring as the batch dict ``grad`` / ``step`` take (views,
        no copy); sample indices below ``size``."""
        return {n: getattr(self, n) for n in BATCH_FIELDS}

    def sample(self, n, generator=None):
        """``n`` int32 indices in ``[0, size)`` on the memory's device, from
        one ``torch.randint``."""
        import torch
        n = int(n)
        if n < 1:
            raise ValueError('n must be >= 1, got %d' % n)
        if self.size < 1:
            raise ValueError('the memory is empty')
        return torch.randint(0, self.size, (n,), dtype=torch.int32, device=self.obs0.device,
                             generator=generator)
