"""The PPO2 learner on the device: GAE, the loss gradient and the Adam step of
stable-baselines 2.x ``PPO2`` over ``MlpPolicy`` as HIP kernels (``ce_ppo2_*``,
csrc/ppo2_kernels.h), so collect -> gae -> update -> collect needs no eager
torch and no host round trip.

The three ``*_numpy`` functions are the executable statement of the semantics
(any dtype, no GPU) and the checkers of the kernels:

    gae_numpy        delta_t = r_t + gamma V_{t+1} (1 - done_t) - V_t
                     adv_t   = delta_t + gamma lam (1 - done_t) adv_{t+1}
                     returns = adv + values
    loss_grad_numpy  z = (a - mean) / std, std = exp(logstd)
                     neglogp = 0.5 sum z^2 + sum logstd + 0.5 A log 2 pi
                     ratio   = exp(old_neglogp - neglogp)
                     pg = mean(max(-adv ratio, -adv clip(ratio, 1 - c, 1 + c)))
                     vf = 0.5 mean(max((v - R)^2, (vclip - R)^2))
                     loss = pg - ent_coef entropy + vf_coef vf
                     and d loss / d params by hand-written backprop
    adam_step_numpy  TF's clip_by_global_norm, then TF-style Adam

``neglogp`` here is the true density of the stored *unclipped* action under
the current parameters, not the rollout's noise form: the parameters have
moved since the action was drawn.

``adv_moments_numpy`` and ``merge_moments_numpy`` state how ranks that
exchange gradients (``distributed.GradientExchange``) normalise advantages
over all their rows: per-rank two-pass moments, merged in rank order.

``PPO2Learner`` owns the master flat parameters, Adam's ``m`` / ``v`` and the
step count on the policy's device and writes every update through to the
policy's image, so the next ``forward_device`` / ``rollout_policy`` sees it.
"""
from collections import namedtuple

import numpy as np

from custom_envs_amd import learner
from custom_envs_amd._native import CePpo2Config
from custom_envs_amd.learner import N_STATS  # noqa: F401  (part of this module's names)
from custom_envs_amd.learner import (Learner, check_rate, clip_by_global_norm_numpy, gaussian_head,
                                     gaussian_head_backward, mlp_backward, mlp_forward,
                                     statement_inputs)
from custom_envs_amd.policy import dict_to_flat

# the first six of the N_STATS (8) floats a call writes; then ||grad||^2, one spare
STAT_NAMES = ('loss', 'pg_loss', 'vf_loss', 'entropy', 'approxkl', 'clipfrac')

HyperParams = namedtuple('HyperParams', 'cliprange cliprange_vf ent_coef vf_coef normalize_adv')
HyperParams.__new__.__defaults__ = (0.2, None, 0.01, 0.5, True)


# ------------------------------------------------------------------ statements
def gae_numpy(rewards, values, dones, last_values, gamma=0.99, lam=0.95, dtype=np.float64):
    """Generalised advantage estimation over ``[K][R]`` arrays in ``dtype``.
    ``dones[t]`` is the flag step t returned (what ``collect`` stores), so
    ``nonterminal_t = 1 - dones[t]``.  Returns (advantages, returns)."""
    rewards = np.asarray(rewards, dtype)
    values = np.asarray(values, dtype)
    nonterminal = dtype(1) - (np.asarray(dones) != 0).astype(dtype)
    last_values = np.asarray(last_values, dtype)
    gamma, gl = dtype(gamma), dtype(gamma) * dtype(lam)
    K = rewards.shape[0]
    adv = np.zeros_like(rewards)
    carry = np.zeros_like(last_values)
    for t in range(K - 1, -1, -1):
        v_next = last_values if t == K - 1 else values[t + 1]
        delta = rewards[t] + gamma * v_next * nonterminal[t] - values[t]
        carry = delta + gl * nonterminal[t] * carry
        adv[t] = carry
    return adv, adv + values


def loss_grad_numpy(params, obs, actions, advantages, returns, old_neglogp, old_values,
                    hp=HyperParams(), hidden=(64, 64), dtype=np.float64):
    """The PPO2 loss and its gradient in ``dtype`` (manual backprop, NumPy
    only).  ``params``: the flat vector or the ``params_layout`` dict.
    Returns (stats dict of STAT_NAMES, grad in the flat ``params_layout``
    order).  ``hp.cliprange_vf`` None means ``hp.cliprange``; negative means
    no value clipping."""
    obs, actions, layout, p = statement_inputs(params, obs, actions, hidden, dtype)
    N = actions.shape[0]
    adv = np.asarray(advantages, dtype)
    returns = np.asarray(returns, dtype)
    old_neglogp = np.asarray(old_neglogp, dtype)
    old_values = np.asarray(old_values, dtype)
    c = dtype(hp.cliprange)
    cv = c if hp.cliprange_vf is None else dtype(hp.cliprange_vf)
    L = len(hidden)
    grad = {}

    if hp.normalize_adv:
        adv = (adv - adv.mean()) / (adv.std() + dtype(1e-8))

    # the policy network
    xs, mean = mlp_forward(p, 'pi', obs, L)
    z, std, neglogp, entropy = gaussian_head(p['logstd'], actions, mean, dtype)
    ratio = np.exp(old_neglogp - neglogp)
    pg1 = -adv * ratio
    pg2 = -adv * np.clip(ratio, dtype(1) - c, dtype(1) + c)
    pg_loss = np.mean(np.maximum(pg1, pg2))
    inside = (ratio > dtype(1) - c) & (ratio < dtype(1) + c)
    # d term / d neglogp: d ratio / d neglogp = -ratio
    w_pg = np.where((pg1 >= pg2) | inside, adv * ratio, dtype(0)) / dtype(N)
    gaussian_head_backward(p, grad, xs, z, std, w_pg, dtype(hp.ent_coef), dtype)

    # the value network
    xs, vout = mlp_forward(p, 'vf', obs, L)
    vpred = vout[:, 0]
    e1 = vpred - returns
    if cv < 0:
        vf_loss = dtype(0.5) * np.mean(e1 * e1)
        dv = e1
    else:
        diff = vpred - old_values
        e2 = old_values + np.clip(diff, -cv, cv) - returns
        vf_loss = dtype(0.5) * np.mean(np.maximum(e1 * e1, e2 * e2))
        dv = np.where(e1 * e1 >= e2 * e2, e1, np.where(np.abs(diff) < cv, e2, dtype(0)))
    mlp_backward(p, grad, 'vf', xs, (dtype(hp.vf_coef) * dv / dtype(N))[:, None], dtype)

    stats = {
        'loss': pg_loss - dtype(hp.ent_coef) * entropy + dtype(hp.vf_coef) * vf_loss,
        'pg_loss': pg_loss, 'vf_loss': vf_loss, 'entropy': entropy,
        'approxkl': dtype(0.5) * np.mean((neglogp - old_neglogp) ** 2),
        'clipfrac': np.mean((np.abs(ratio - dtype(1)) > c).astype(dtype)),
    }
    return stats, dict_to_flat(grad, layout, dtype)


def adam_step_numpy(params, grad, m, v, t, lr, max_grad_norm=0.5, beta1=0.9, beta2=0.999,
                    eps=1e-5):
    """One update in the arrays' dtype; ``t`` is the 1-based step count.
    Returns (params, m, v), all new arrays.

    With ``max_grad_norm > 0`` the gradient is first scaled by
    ``min(1, max_grad_norm / (||grad||_2 + 1e-6))``: TF's
    ``clip_by_global_norm`` up to the 1e-6 in the denominator, which keeps a
    zero gradient finite.  Then TF-style Adam, the bias correction folded
    into the step size and epsilon outside it:

        lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t)
        m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2
        params -= lr_t m / (sqrt(v) + eps)
    """
    params, grad, m, v = (np.asarray(a) for a in (params, grad, m, v))
    dt = params.dtype.type
    grad = clip_by_global_norm_numpy(grad, max_grad_norm, dt)
    m = dt(beta1) * m + dt(1 - beta1) * grad
    v = dt(beta2) * v + dt(1 - beta2) * grad * grad
    lr_t = dt(lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t))
    return params - lr_t * m / (np.sqrt(v) + dt(eps)), m, v


def adv_moments_numpy(advantages):
    """What ``ppo2_advmoments_kernel`` leaves for one rank: ``(n, mean, M2 =
    sum (a - mean)^2)`` in float64, by the two-pass formula."""
    a = np.asarray(advantages, np.float64).reshape(-1)
    mean = a.sum() / a.size
    d = a - mean
    return np.array([a.size, mean, np.sum(d * d)], np.float64)


def merge_moments_numpy(moments):
    """The statement of ``ppo2_advmerge_kernel``: the ranks' ``[W][3]``
    triples merged in rank order by Chan's formula.  Returns ``(mean, 1 /
    (sqrt(M2 / N) + 1e-8))`` in float64: the normalisation of all N
    advantages.  One triple passes through untouched."""
    moments = np.asarray(moments, np.float64).reshape(-1, 3)
    cnt, mean, m2 = moments[0]
    for nr, mean_r, m2_r in moments[1:]:
        delta = mean_r - mean
        tot = cnt + nr
        mean = mean + delta * nr / tot
        m2 = m2 + m2_r + delta * delta * cnt * nr / tot
        cnt = tot
    return mean, 1.0 / (np.sqrt(m2 / cnt) + 1e-8)


# --------------------------------------------------------------------- learner
class Stats(learner.Stats):
    """The statistics of one ``grad`` / ``step`` call as a device tensor
    (``.tensor``: STAT_NAMES, then ||grad||^2); ``.stats()`` copies them out."""
    names = STAT_NAMES


BATCH_FIELDS = ('obs', 'actions', 'advantages', 'returns', 'neglogps', 'values')


class PPO2Learner(Learner):
    """PPO2's learner for one ``MlpPolicy`` (see the module docstring).  A
    policy built with ``device=None`` gives the shape-and-validation-only
    form, which needs no GPU.  Hyper-parameters are stable-baselines'
    defaults; ``cliprange_vf`` None means ``cliprange``, negative means no
    value clipping; ``grid_limit`` 0 means one workgroup per CU per network.
    ``set_params`` keeps Adam's moments and step count."""
    PREFIX = 'ce_ppo2'
    CONFIG = CePpo2Config
    BATCH_FIELDS = BATCH_FIELDS
    STATS = Stats
    OPT_BLOCKS = ('m', 'v')      # Adam's moments; ``step`` counts its steps
    _loss_grad = staticmethod(loss_grad_numpy)

    def __init__(self, policy, gamma=0.99, lam=0.95, cliprange=0.2, cliprange_vf=None,
                 ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5, lr=2.5e-4, beta1=0.9,
                 beta2=0.999, eps=1e-5, normalize_adv=True, grid_limit=0):
        super().__init__(
            policy, gamma=gamma, lam=lam, cliprange=cliprange,
            cliprange_vf=cliprange if cliprange_vf is None else cliprange_vf,
            ent_coef=ent_coef, vf_coef=vf_coef, max_grad_norm=max_grad_norm, lr=lr, beta1=beta1,
            beta2=beta2, eps=eps, normalize_adv=int(bool(normalize_adv)), grid_limit=int(grid_limit))
        self.hp = HyperParams(cliprange, cliprange_vf, ent_coef, vf_coef, bool(normalize_adv))
        self.lam = float(lam)

    def gae(self, result=None, rewards=None, values=None, dones=None, last_values=None,
            stream=None):
        """Advantages and returns, ``[K][R]`` contiguous float32 device
        tensors, of the dict ``collect`` returns (or of the four tensors
        given by name).  ``rewards`` / ``dones`` / ``values`` are read in
        place in the strided rollout records; nothing is copied."""
        import torch
        if result is not None:
            rewards, values = result['rewards'], result['values']
            dones, last_values = result['dones'], result['last_values']
        k, rows = self.rollout_shape(rewards)
        self.check_records('rewards', rewards, torch.float32, k, rows)
        self.check_records('values', values, torch.float32, k, rows)
        self.check_records('dones', dones, torch.uint8, k, rows)
        self.policy.check_input('last_values', last_values, (rows,), placement=False)
        for name, t in (('rewards', rewards), ('values', values), ('dones', dones),
                        ('last_values', last_values)):
            self.policy.check_device(name, t)
        adv = torch.empty((k, rows), dtype=torch.float32, device=rewards.device)
        ret = torch.empty_like(adv)
        stride = self._stride_bytes
        self._call('gae', self._h, k, rows, rewards.data_ptr(), stride(rewards), dones.data_ptr(),
                   stride(dones), values.data_ptr(), stride(values), last_values.data_ptr(),
                   adv.data_ptr(), ret.data_ptr(), self._stream(stream))
        return adv, ret

    # ---------------------------------------------------------- gradient, step
    def grad(self, batch, idx=None, stream=None, cliprange=None):
        """The loss gradient of the rows ``idx`` (None: all) of ``batch``, no
        update.  ``cliprange`` as in ``step``.  Returns (grad ``[n_params]``
        device tensor, ``Stats``)."""
        import torch
        clip = check_rate('cliprange', cliprange)
        if self.exchange is not None:      # the gradient of every rank's rows
            records, n_total = self._exchange_records(batch, idx, stream, cliprange)
            return self.combine(records, n_total, stream=stream)
        head, stats = self._head(batch, idx)
        grad = torch.empty(self.n_params, dtype=torch.float32, device=stats.device)
        self._call('grad', *head, clip, grad.data_ptr(),
                   stats.data_ptr(), self._stream(stream))
        return grad, Stats(stats)

    # ------------------------------------------------------- gradient exchange
    def adv_moments(self, batch, idx=None, out=None, stream=None):
        """``(n, mean, M2)`` of the advantages of the rows ``idx`` (None: all)
        as three float64 on the device (``out`` or a new tensor): this rank's
        share of the global normalisation (``merge_moments_numpy``)."""
        import torch
        M, N = self.check_batch(batch, idx)
        if out is None:
            out = torch.zeros(3, dtype=torch.float64, device=batch['obs'].device)
        else:
            self.check_record_tensor('out', out, (3,))
        self._call('adv_moments', self._h, N, M, None if idx is None else idx.data_ptr(),
                   batch['advantages'].data_ptr(), out.data_ptr(), self._stream(stream))
        return out

    def partial(self, batch, idx=None, n_total=None, moments=None, out=None, stream=None,
                cliprange=None):
        """This rank's share of a step of ``n_total`` rows (None: its own
        ``n``): the gradient of the rows ``idx`` with the row weight ``1 /
        n_total``, normalised by the merged ``moments`` (``[world][3]``
        float64, every rank's ``adv_moments``; None with ``n_total == n``:
        this call's own), as one float64 record in ``out`` (``[record_doubles]``;
        None: a new tensor).  ``cliprange`` as in ``step``.  Returns the
        record."""
        cliprange = check_rate('cliprange', cliprange)
        n_total = self.check_total(self._rows_of(batch, idx), n_total)
        if out is not None:
            self.check_record_tensor('out', out, (self.record_doubles,))
        M, N = self.check_batch(batch, idx)
        world = 1
        if not self.hp.normalize_adv:
            moments = None
        elif moments is None:
            if n_total != N:
                raise ValueError('moments of every rank are needed to normalise over n_total = %d '
                                 'rows (this call has %d)' % (n_total, N))
            moments = self.adv_moments(batch, idx, stream=stream).reshape(1, 3)
        else:
            if not hasattr(moments, 'dim') or moments.dim() != 2:
                raise ValueError('moments must have shape [world][3]')
            world = int(moments.shape[0])
            self.check_record_tensor('moments', moments, (world, 3))
        out = self._record_out(out, batch['obs'])
        ptrs = [batch[n].data_ptr() for n in self.BATCH_FIELDS]
        self._call('partial', self._h, N, n_total, M, None if idx is None else idx.data_ptr(),
                   *ptrs, cliprange, world,
                   None if moments is None else moments.data_ptr(), out.data_ptr(),
                   self._stream(stream))
        return out

    def _exchange_records(self, batch, idx, stream, cliprange):
        """partial, the gather(s): (the gathered records, n_total)."""
        ex = self.exchange
        n_total = ex.total_rows(self._rows_of(batch, idx))
        moments = None
        if self.hp.normalize_adv:
            self.adv_moments(batch, idx, out=ex.moments[ex.rank], stream=stream)
            moments = ex.gather_moments()
        self.partial(batch, idx, n_total=n_total, moments=moments, out=ex.records[ex.rank],
                     stream=stream, cliprange=cliprange)
        return ex.gather_records(), n_total

    def step(self, batch, idx=None, stream=None, lr=None, cliprange=None):
        """Gradient, global-norm clip, Adam and the policy image's repack as
        one stream-ordered call.  ``lr`` / ``cliprange`` override the
        learner's for this call: None means the learner's own, a finite
        positive number is used, and anything else (0.0 from a schedule, a
        negative number, NaN, inf) raises ``ValueError`` before any device
        call.  Returns ``Stats``.  With a gradient exchange attached it is
        the step on every rank's rows: [moments, gather,] partial, gather,
        apply."""
        rate, clip = check_rate('lr', lr), check_rate('cliprange', cliprange)
        if self.exchange is not None:
            records, n_total = self._exchange_records(batch, idx, stream, cliprange)
            return self.apply(records, n_total, lr=lr, stream=stream)
        head, stats = self._head(batch, idx)
        self._call('step', *head, rate, clip, stats.data_ptr(), self._stream(stream))
        self.policy._host_params = None
        return Stats(stats)

    def flatten(self, result, advantages, returns):
        """The ``[K R]`` batch of a ``collect`` result and its GAE outputs
        (the strided policy records made contiguous once, on the device)."""
        k, rows = (int(s) for s in result['rewards'].shape)
        return {'obs': result['obs'].reshape(k * rows, -1).contiguous(),
                'actions': result['actions'].reshape(k * rows, -1).contiguous(),
                'advantages': advantages.reshape(-1), 'returns': returns.reshape(-1),
                'neglogps': result['neglogps'].reshape(-1).contiguous(),
                'values': result['values'].reshape(-1).contiguous()}

    def check_perms(self, perms, noptepochs, total):
        """``perms``: ``noptepochs`` int32 contiguous ``[total]`` tensors (the
        device is checked with the batch, by ``step``)."""
        import torch
        perms = list(perms)
        if len(perms) != noptepochs:
            raise ValueError('perms holds %d permutations, noptepochs is %d'
                             % (len(perms), noptepochs))
        for i, perm in enumerate(perms):
            if not hasattr(perm, 'data_ptr') or perm.dtype != torch.int32:
                raise ValueError('perms[%d] must be an int32 tensor, got %s'
                                 % (i, getattr(perm, 'dtype', type(perm).__name__)))
            if tuple(perm.shape) != (total,) or not perm.is_contiguous():
                raise ValueError('perms[%d] must be contiguous with shape (%d,), got %s'
                                 % (i, total, tuple(perm.shape)))
        return perms

    def update(self, result, noptepochs=4, nminibatches=4, generator=None, lr=None,
               cliprange=None, stream=None, perms=None):
        """The whole PPO2 update of one rollout: GAE, then ``noptepochs``
        passes of ``nminibatches`` ``step`` calls over slices of one
        ``torch.randperm`` per epoch (drawn on the device from ``generator``),
        or of ``perms[epoch]`` when ``perms`` is given: ``noptepochs`` int32
        device permutations of the ``K * R`` rows (``rng.DeviceRng.
        permutation``), so the split does not depend on torch's generator.
        ``lr`` / ``cliprange`` reach every minibatch step and are checked as
        ``step`` checks them, before anything else.
        Nothing is read back; returns the ``Stats`` of every step, in order.
        With a gradient exchange attached every rank splits its own ``K * R_r``
        rows with its own ``generator``, and ``K * R_r`` must divide by
        ``nminibatches`` on every rank (checked on every rank, before any
        launch)."""
        import torch
        check_rate('lr', lr)
        check_rate('cliprange', cliprange)
        for name in ('obs', 'actions', 'values', 'neglogps', 'rewards', 'dones', 'last_values'):
            if result.get(name) is None:
                raise ValueError('result lacks %r' % name)
        noptepochs, nminibatches = int(noptepochs), int(nminibatches)
        if noptepochs < 1 or nminibatches < 1:
            raise ValueError('noptepochs and nminibatches must be >= 1')
        k, rows = self.rollout_shape(result['rewards'])
        total = k * rows
        if total % nminibatches:
            raise ValueError('K * R = %d rows do not split into %d minibatches'
                             % (total, nminibatches))
        if perms is not None:
            perms = self.check_perms(perms, noptepochs, total)
        if self.exchange is not None:
            # decided for every rank on every rank, so none enters a
            # collective alone
            self.exchange.check_rows(rows)
            for r, c in enumerate(self.exchange.counts):
                if (k * c) % nminibatches:
                    raise ValueError('rank %d: K * R = %d rows do not split into %d minibatches'
                                     % (r, k * c, nminibatches))
        for name, tail in (('obs', (self.policy.obs_dim,)), ('actions', (self.policy.act_dim,)),
                           ('neglogps', ())):
            t = result[name]
            if t.dtype != torch.float32:
                raise ValueError('%s must have dtype float32, got %s' % (name, t.dtype))
            if tuple(t.shape) != (k, rows) + tail:
                raise ValueError('%s must have shape %s, got %s'
                                 % (name, (k, rows) + tail, tuple(t.shape)))
        adv, ret = self.gae(result, stream=stream)
        self.last_returns = ret      # [K][R], for a caller's explained variance
        batch = self.flatten(result, adv, ret)
        self.check_batch(batch)
        size = total // nminibatches
        all_stats = []
        for epoch in range(noptepochs):
            if perms is not None:
                perm = perms[epoch]
            else:
                perm = torch.randperm(total, dtype=torch.int32, device=adv.device,
                                      generator=generator)
            for b in range(nminibatches):
                all_stats.append(self.step(batch, perm[b * size:(b + 1) * size], stream=stream,
                                           lr=lr, cliprange=cliprange))
        return all_stats


class WidePPO2Learner(PPO2Learner):
    """``PPO2Learner`` for one ``WideMlpPolicy`` (obs_dim <= 1024, act_dim <=
    512): ``ce_ppo2_create_wide``, whose gradient runs on the chunked kernel of
    csrc/ppo_grad_wide_tile.h.  Everything else is ``PPO2Learner``'s; at a shape
    ``PPO2Learner`` takes too, gradients (but dlogstd's last place) and
    statistics are the same bits at the same ``grid_limit`` (0 here means 64
    workgroups per network)."""
    WIDE = True
