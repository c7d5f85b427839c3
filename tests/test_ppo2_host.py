"""The PPO2 learner without a GPU: the NumPy statements of custom_envs_amd/ppo2.py
against independent restatements, the C argument checks of ce_ppo2_* (all
before the first HIP call) and PPO2Learner's tensor validation.

1. ``loss_grad_numpy`` (hand-written backprop) in float64 against torch
   autograd on a torch restatement of the loss written here, every case of
   ppo2_cases (CASES and SHAPE_CASES): gradient and every statistic within
   1e-9 norm-relative.  ``ppo2_cases.net_errs`` refuses a 1e-4 relative error
   of the value network that ``block_errs`` lets through.
2. ``gae_numpy`` against a literal loop, an episode end in the middle and at
   t = K - 1.
3. ``adam_step_numpy`` against TF-style Adam restated with torch tensors over
   3 steps, the norm clip active and inactive.
4. Every bad argument of the C entry points: CE_EINVAL naming it.
5. ``PPO2Learner`` validation on CPU tensors: a named ValueError each.
"""
import ctypes

import numpy as np
import pytest

import ppo2_cases as cases
from custom_envs_amd import _native
from custom_envs_amd.policy import MlpPolicy, params_layout
from custom_envs_amd.ppo2 import (STAT_NAMES, HyperParams, PPO2Learner, adam_step_numpy,
                                  gae_numpy, loss_grad_numpy)

BOUND = 1e-9


# ----------------------------------------------------- 1. the gradient statement
def _torch_loss(case, inputs, hp):
    import torch
    N, D, hidden, A, _ = case
    layout = params_layout(D, A, hidden)
    flat = torch.tensor(inputs['params'], dtype=torch.float64, requires_grad=True)
    p = {name: flat[off:off + int(np.prod(shape))].reshape(shape)
         for name, (off, shape) in layout.items()}
    t = {n: torch.tensor(inputs[n], dtype=torch.float64) for n in cases.BATCH_FIELDS}

    def mlp(net):
        x = t['obs']
        for i in range(len(hidden)):
            x = torch.tanh(x @ p['%s/w%d' % (net, i)] + p['%s/b%d' % (net, i)])
        return x @ p['%s/w_out' % net] + p['%s/b_out' % net]

    mean, vpred = mlp('pi'), mlp('vf')[:, 0]
    logstd = p['logstd']
    neglogp = (0.5 * (((t['actions'] - mean) / torch.exp(logstd)) ** 2).sum(1) + logstd.sum()
               + 0.5 * A * np.log(2 * np.pi))
    entropy = (logstd + 0.5 * np.log(2 * np.pi * np.e)).sum()
    adv = t['advantages']
    if hp.normalize_adv:
        adv = (adv - adv.mean()) / (adv.std(unbiased=False) + 1e-8)
    ratio = torch.exp(t['neglogps'] - neglogp)
    c = hp.cliprange
    pg = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - c, 1 + c)).mean()
    cv = c if hp.cliprange_vf is None else hp.cliprange_vf
    if cv < 0:
        vf = 0.5 * ((vpred - t['returns']) ** 2).mean()
    else:
        vclip = t['values'] + torch.clamp(vpred - t['values'], -cv, cv)
        vf = 0.5 * torch.max((vpred - t['returns']) ** 2, (vclip - t['returns']) ** 2).mean()
    loss = pg - hp.ent_coef * entropy + hp.vf_coef * vf
    loss.backward()
    stats = {'loss': loss, 'pg_loss': pg, 'vf_loss': vf, 'entropy': entropy,
             'approxkl': 0.5 * ((neglogp - t['neglogps']) ** 2).mean(),
             'clipfrac': ((ratio - 1).abs() > c).double().mean()}
    return {k: float(v.detach()) for k, v in stats.items()}, flat.grad.numpy()


@pytest.mark.parametrize('hp', [cases.HP, cases.HP._replace(cliprange_vf=-1.0, normalize_adv=False),
                                cases.HP._replace(cliprange_vf=None)],
                         ids=['default', 'no_vclip_no_norm', 'vclip_from_cliprange'])
@pytest.mark.parametrize('case', cases.CASES + cases.SHAPE_CASES,
                         ids=cases.CASE_IDS + cases.SHAPE_CASE_IDS)
def test_loss_grad_numpy_against_autograd(case, hp):
    inputs = cases.inputs_of(case)
    ref_stats, ref_grad = _torch_loss(case, inputs, hp)
    stats, grad = loss_grad_numpy(inputs['params'], *[inputs[n] for n in cases.BATCH_FIELDS],
                                  hp=hp, hidden=inputs['hidden'], dtype=np.float64)
    assert grad.dtype == np.float64 and grad.shape == ref_grad.shape
    err = np.linalg.norm(grad - ref_grad) / np.linalg.norm(ref_grad)
    print('loss_grad_numpy', case, err)
    assert err <= BOUND
    assert set(stats) == set(STAT_NAMES)
    for name in STAT_NAMES:
        assert abs(float(stats[name]) - ref_stats[name]) <= BOUND * max(abs(ref_stats[name]), 1e-300), name


def test_loss_grad_numpy_runs_in_float32():
    inputs = cases.draw_case(cases.CASES[2])
    args = [inputs[n] for n in cases.BATCH_FIELDS]
    stats, grad = loss_grad_numpy(inputs['params'], *args, hp=cases.HP, hidden=inputs['hidden'],
                                  dtype=np.float32)
    _, ref = loss_grad_numpy(inputs['params'], *args, hp=cases.HP, hidden=inputs['hidden'])
    assert grad.dtype == np.float32 and all(np.asarray(v).dtype == np.float32 for v in stats.values())
    assert np.max(np.abs(grad - ref)) / np.max(np.abs(ref)) <= 1e-4


def test_case_generator_covers_both_branches():
    """What draw_case asserts, seen from outside: margins and branch shares."""
    for case in cases.CASES + cases.SHAPE_CASES:
        inputs = cases.inputs_of(case)
        assert all(inputs[n].dtype == np.float32 for n in cases.BATCH_FIELDS)
        assert np.any(np.abs(inputs['obs']) > 50) or case[0] < 8       # saturated rows
        assert inputs['hidden'] == case[2] and inputs['grid_limit'] == case[4]


def test_pg_terms_are_pg_loss_and_cases_do_not_cancel():
    """``pg_terms`` restates the statement's pg_loss row by row, and on CASES
    its condition number stays below ``PG_COND_MAX``: test_gpu_ppo2.py holds
    pg_loss to 1e-5 of itself there.  Three of the SHAPE_CASES cancel."""
    cancelling = []
    for case in cases.CASES + cases.SHAPE_CASES:
        inputs = cases.inputs_of(case)
        for hp in (cases.HP, cases.HP._replace(cliprange_vf=-1.0, normalize_adv=False)):
            stats, _ = loss_grad_numpy(inputs['params'], *[inputs[n] for n in cases.BATCH_FIELDS],
                                       hp=hp, hidden=inputs['hidden'])
            terms = cases.pg_terms(inputs, hp)
            assert terms.shape == (case[0],)
            assert abs(terms.mean() - float(stats['pg_loss'])) <= 1e-12 * max(np.abs(terms).mean(), 1e-300)
        terms = cases.pg_terms(inputs)
        pg = float(terms.mean())
        cond = float(np.abs(terms).mean() / abs(pg)) if pg != 0.0 else 0.0
        print(case, 'pg_loss %.4g condition %.1f' % (pg, cond))
        if case in cases.CASES:
            assert cond <= cases.PG_COND_MAX, (case, cond)
        elif cond > cases.PG_COND_MAX:
            cancelling.append(case[2])
    assert cancelling == [(32, 128), (96, 96), (64, 96, 128)]


def test_net_errs_sees_what_block_errs_hides():
    """A 1e-4 relative error over the whole value network passes ``block_errs``
    at 1e-5, because that measure divides by the largest entry of the whole
    gradient, the policy network's, and the value network's entries are 25
    times smaller on this case; ``net_errs`` divides by the network's own
    largest entry, and its bound (twice the float32 statement's own error, at
    least 1e-5) refuses it."""
    case = cases.CASES[4]
    inputs = cases.inputs_of(case)
    args = [inputs[n] for n in cases.BATCH_FIELDS]
    _, ref = loss_grad_numpy(inputs['params'], *args, hp=cases.HP, hidden=inputs['hidden'])
    _, g32 = loss_grad_numpy(inputs['params'], *args, hp=cases.HP, hidden=inputs['hidden'],
                             dtype=np.float32)
    wrong = ref.copy()
    for name, sl in cases.blocks(case).items():
        if name.startswith('vf/'):
            wrong[sl] *= 1.0 + 1e-4
    old, new = cases.block_errs(case, wrong, ref), cases.net_errs(case, wrong, ref)
    bounds = cases.net_bounds(case, g32, ref)
    print('block_errs worst %.3g, net_errs %s, bounds %s' % (max(old.values()), new, bounds))
    assert set(new) == set(bounds) == {'pi', 'vf', 'logstd'}
    assert max(old.values()) <= 1e-5                        # the gap
    assert new['vf'] == pytest.approx(1e-4, rel=1e-6) and new['vf'] > bounds['vf']
    assert new['pi'] == 0.0 and new['logstd'] == 0.0
    # the bound is the reference's: twice the float32 statement's own error
    e32 = cases.net_errs(case, g32, ref)
    assert bounds == {net: max(1e-5, 2.0 * e) for net, e in e32.items()}
    # a network whose reference is all zero is measured on the whole gradient's scale
    one = cases.CASES[0]
    inp = cases.inputs_of(one)
    _, ref1 = loss_grad_numpy(inp['params'], *[inp[n] for n in cases.BATCH_FIELDS], hp=cases.HP,
                              hidden=inp['hidden'])
    sl = cases.blocks(one)['vf/w0']
    assert not ref1[sl].any()
    off = ref1.copy()
    off[sl.start] = 1e-3 * np.abs(ref1).max()
    assert cases.net_errs(one, off, ref1)['vf'] == pytest.approx(1e-3)


# ------------------------------------------------------------------------ 2. GAE
def test_gae_numpy_against_literal_loop():
    rs = np.random.RandomState(3)
    K, R, gamma, lam = 7, 5, 0.99, 0.95
    rewards, values = rs.normal(0, 1, (K, R)), rs.normal(0, 1, (K, R))
    last_values = rs.normal(0, 1, R)
    dones = np.zeros((K, R), np.uint8)
    dones[3, 0] = dones[K - 1, 1] = dones[2, 2] = dones[K - 1, 2] = 1
    adv = np.zeros((K, R))
    for r in range(R):
        carry = 0.0
        for t in reversed(range(K)):
            nt = 1.0 - dones[t, r]
            v_next = last_values[r] if t == K - 1 else values[t + 1, r]
            carry = rewards[t, r] + gamma * v_next * nt - values[t, r] + gamma * lam * nt * carry
            adv[t, r] = carry
    got_adv, got_ret = gae_numpy(rewards, values, dones, last_values, gamma, lam)
    assert np.allclose(got_adv, adv, rtol=1e-13, atol=1e-13)
    assert np.allclose(got_ret, adv + values, rtol=1e-13, atol=1e-13)
    # an episode end cuts the bootstrap and the carry
    assert got_adv[K - 1, 1] == rewards[K - 1, 1] - values[K - 1, 1]
    assert got_adv[3, 0] == rewards[3, 0] - values[3, 0]
    a32, r32 = gae_numpy(rewards, values, dones, last_values, gamma, lam, dtype=np.float32)
    assert a32.dtype == np.float32 and r32.dtype == np.float32
    assert np.allclose(a32, adv, rtol=1e-5, atol=1e-5)


# ----------------------------------------------------------------------- 3. Adam
@pytest.mark.parametrize('max_grad_norm', [0.5, 1e6, 0.0], ids=['clip_bites', 'clip_idle', 'no_clip'])
def test_adam_step_numpy_against_tf_style_restatement(max_grad_norm):
    """torch.optim.Adam divides by sqrt(v_hat) + eps; TF (and stable-baselines)
    fold the bias correction into the step size and add eps to sqrt(v).  The
    restatement below is TF's, in torch tensors."""
    import torch
    rs = np.random.RandomState(4)
    n, lr, b1, b2, eps = 50, 3e-3, 0.9, 0.999, 1e-5
    p0 = rs.normal(0, 1, n)
    grads = [rs.normal(0, 1, n) for _ in range(3)]
    p, m, v = torch.tensor(p0), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    q, qm, qv = p0.copy(), np.zeros(n), np.zeros(n)
    for t, g in enumerate(grads, 1):
        gt = torch.tensor(g)
        if max_grad_norm > 0:
            norm = torch.sqrt((gt * gt).sum())
            gt = gt * torch.clamp(max_grad_norm / (norm + 1e-6), max=1.0)
            assert (float(norm) > max_grad_norm) == (max_grad_norm == 0.5)
        m = b1 * m + (1 - b1) * gt
        v = b2 * v + (1 - b2) * gt * gt
        p = p - lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t) * m / (torch.sqrt(v) + eps)
        q, qm, qv = adam_step_numpy(q, g, qm, qv, t, lr, max_grad_norm, b1, b2, eps)
        assert np.linalg.norm(q - p.numpy()) <= BOUND * np.linalg.norm(p.numpy())
        assert np.linalg.norm(qm - m.numpy()) <= BOUND * np.linalg.norm(m.numpy())
        assert np.linalg.norm(qv - v.numpy()) <= BOUND * np.linalg.norm(v.numpy())


# ------------------------------------------------------ 4. the C argument checks
def _cfg(**over):
    base = dict(gamma=0.99, lam=0.95, cliprange=0.2, cliprange_vf=0.2, ent_coef=0.01, vf_coef=0.5,
                max_grad_norm=0.5, lr=2.5e-4, beta1=0.9, beta2=0.999, eps=1e-5, normalize_adv=1,
                grid_limit=0)
    base.update(over)
    return _native.CePpo2Config(**base)


def _refused(rc, word):
    msg = _native.load().ce_last_error().decode()
    assert rc == _native.CE_EINVAL, (rc, msg)
    assert word in msg, msg


def test_new_symbols_are_exported():
    lib = _native.load()
    for name in ('ce_ppo2_create', 'ce_ppo2_destroy', 'ce_ppo2_set_params', 'ce_ppo2_get_params',
                 'ce_ppo2_gae', 'ce_ppo2_grad', 'ce_ppo2_step'):
        assert name in _native.EXPORTS and hasattr(lib, name), name
    assert lib.ce_abi_version() == 5


@pytest.mark.parametrize('over, word', [
    (dict(gamma=1.5), 'gamma'), (dict(gamma=-0.1), 'gamma'), (dict(gamma=float('nan')), 'gamma'),
    (dict(lam=1.01), 'lam'), (dict(lam=-1.0), 'lam'),
    (dict(cliprange=0.0), 'cliprange'), (dict(cliprange=-0.2), 'cliprange'),
    (dict(cliprange_vf=float('nan')), 'cliprange_vf'), (dict(ent_coef=float('inf')), 'ent_coef'),
    (dict(max_grad_norm=float('nan')), 'max_grad_norm'), (dict(lr=0.0), 'lr'),
    (dict(beta1=1.0), 'beta1'), (dict(beta2=-0.1), 'beta2'), (dict(eps=0.0), 'eps'),
    (dict(grid_limit=-1), 'grid_limit')], ids=lambda v: None if isinstance(v, str) else
    '%s=%s' % next(iter(v.items())))
def test_create_refuses_bad_hyperparameters(over, word):
    """Before the policy handle is looked at: a NULL policy never gets that far."""
    lib = _native.load()
    handle = ctypes.c_void_p()
    cfg = _cfg(**over)
    _refused(lib.ce_ppo2_create(None, ctypes.byref(cfg), ctypes.byref(handle)), word)
    assert not handle.value


def test_create_refuses_null_arguments():
    lib = _native.load()
    handle = ctypes.c_void_p()
    cfg = _cfg()
    _refused(lib.ce_ppo2_create(None, ctypes.byref(cfg), ctypes.byref(handle)), 'null policy')
    _refused(lib.ce_ppo2_create(None, None, ctypes.byref(handle)), 'null config')
    _refused(lib.ce_ppo2_create(None, ctypes.byref(cfg), None), 'null output')
    lib.ce_ppo2_destroy(None)       # a no-op


def test_gae_argument_checks():
    lib = _native.load()
    buf = np.zeros(64, np.float32)
    a = buf.ctypes.data

    def call(k=2, rows=4, rewards=a, rs=16, dones=a, ds=4, values=a, vs=16, last=a, adv=a, ret=a):
        return lib.ce_ppo2_gae(None, k, rows, rewards, rs, dones, ds, values, vs, last, adv, ret, None)

    _refused(call(k=0), 'k must')
    _refused(call(rows=0), 'rows must')
    _refused(call(rewards=None), 'null rewards')
    _refused(call(dones=None), 'null dones')
    _refused(call(values=None), 'null values')
    _refused(call(last=None), 'null last_values')
    _refused(call(adv=None), 'null adv')
    _refused(call(ret=None), 'null adv or ret')
    _refused(call(rs=18), 'reward_stride_bytes')
    _refused(call(rs=8), 'reward_stride_bytes')
    _refused(call(vs=17), 'value_stride_bytes')
    _refused(call(ds=3), 'done_stride_bytes')
    _refused(call(rewards=a + 2), '4-byte aligned')
    _refused(call(), 'null learner')


@pytest.mark.parametrize('entry', ['ce_ppo2_grad', 'ce_ppo2_step'])
def test_grad_and_step_argument_checks(entry):
    lib = _native.load()
    buf = np.zeros(64, np.float32)
    a = buf.ctypes.data
    names = ('obs', 'actions', 'advantages', 'returns', 'old_neglogp', 'old_values')

    def call(n=4, m=4, idx=None, stats=a, grad=a, **ptrs):
        p = [ptrs.get(name, a) for name in names]
        if entry == 'ce_ppo2_grad':
            return lib.ce_ppo2_grad(None, n, m, idx, *p, -1.0, grad, stats, None)
        return lib.ce_ppo2_step(None, n, m, idx, *p, -1.0, -1.0, stats, None)

    _refused(call(n=0), 'n must')
    _refused(call(m=0), 'm must')
    _refused(call(n=5, m=4), 'no idx')
    for name in names:
        _refused(call(**{name: None}), 'null ' + name)
    _refused(call(stats=None), 'null stats')
    if entry == 'ce_ppo2_grad':
        _refused(call(grad=None), 'null grad')
    _refused(call(), 'null learner')
    _refused(call(n=8, m=4, idx=a), 'null learner')      # more rows than m is fine with an idx


def test_params_argument_checks():
    lib = _native.load()
    buf = np.zeros(8, np.float32)
    for fn in (lib.ce_ppo2_set_params, lib.ce_ppo2_get_params):
        _refused(fn(None, None, 8, 0, None), 'null parameter vector')
        _refused(fn(None, buf.ctypes.data, 8, 0, None), 'null learner')


# --------------------------------------------------- 5. PPO2Learner's validation
def _learner(**kw):
    return PPO2Learner(MlpPolicy(5, 2, (32,), device=None), **kw)


def _cpu_batch(M=6):
    import torch
    return {'obs': torch.zeros(M, 5), 'actions': torch.zeros(M, 2), 'advantages': torch.zeros(M),
            'returns': torch.zeros(M), 'neglogps': torch.zeros(M), 'values': torch.zeros(M)}


def test_shape_only_learner_needs_no_gpu():
    learner = _learner(cliprange=0.1)
    assert learner._h is None and learner.n_params == learner.policy.n_params
    assert learner.hp == HyperParams(0.1, None, 0.01, 0.5, True)
    with pytest.raises(TypeError, match='MlpPolicy'):
        PPO2Learner(object())


@pytest.mark.parametrize('change, match', [
    (lambda b, t: b.update(obs=b['obs'].double()), 'obs must have dtype float32'),
    (lambda b, t: b.update(actions=t.zeros(6, 3)), r'actions must have shape \(6, 2\)'),
    (lambda b, t: b.update(returns=t.zeros(7)), r'returns must have shape \(6,\)'),
    (lambda b, t: b.update(values=t.zeros(12)[::2]), 'values must be contiguous'),
    (lambda b, t: b.pop('neglogps'), "batch lacks 'neglogps'"),
    (lambda b, t: b.update(obs=t.zeros(6)), r'obs must have shape \[M\]\[5\]'),
    (lambda b, t: None, 'obs must be on device cuda:0'),
], ids=['dtype', 'shape', 'length', 'stride', 'missing', 'rank', 'device'])
def test_batch_validation_names_the_tensor(change, match):
    import torch
    batch = _cpu_batch()
    change(batch, torch)
    with pytest.raises(ValueError, match=match):
        _learner().check_batch(batch)


@pytest.mark.parametrize('idx, match', [
    (lambda t: t.zeros(3, dtype=t.int64), 'idx must have dtype int32'),
    (lambda t: t.zeros((3, 1), dtype=t.int32), 'idx must have shape'),
    (lambda t: t.zeros(6, dtype=t.int32)[::2], 'idx must be contiguous'),
], ids=['dtype', 'shape', 'stride'])
def test_idx_validation(idx, match):
    import torch
    with pytest.raises(ValueError, match=match):
        _learner().check_batch(_cpu_batch(), idx(torch))


@pytest.mark.parametrize('change, match', [
    (lambda r, t: r.update(rewards=t.zeros(4, 3).double()), 'rewards must have dtype'),
    (lambda r, t: r.update(dones=t.zeros(4, 3)), 'dones must have dtype'),
    (lambda r, t: r.update(values=t.zeros(5, 3)), r'values must have shape \(4, 3\)'),
    (lambda r, t: r.update(values=t.zeros(4, 6)[:, ::2]), 'values: every record must be contiguous'),
    (lambda r, t: r.update(last_values=t.zeros(4)), r'last_values must have shape \(3,\)'),
    (lambda r, t: r.update(rewards=t.zeros(3)), r'rewards must have shape \[K\]\[R\]'),
    (lambda r, t: None, 'rewards must be on device cuda:0'),
], ids=['dtype', 'done_dtype', 'shape', 'stride', 'last', 'rank', 'device'])
def test_gae_validation_names_the_tensor(change, match):
    import torch
    result = {'rewards': torch.zeros(4, 3), 'values': torch.zeros(4, 3),
              'dones': torch.zeros(4, 3, dtype=torch.uint8), 'last_values': torch.zeros(3)}
    change(result, torch)
    with pytest.raises(ValueError, match=match):
        _learner().gae(result)


@pytest.mark.parametrize('change, match', [
    (lambda r, t: r.pop('actions'), "result lacks 'actions'"),
    (lambda r, t: r.update(obs=t.zeros(4, 3, 6)), r'obs must have shape \(4, 3, 5\)'),
    (lambda r, t: r.update(neglogps=t.zeros(4, 3).double()), 'neglogps must have dtype float32'),
    (lambda r, t: None, 'rewards must be on device cuda:0'),
], ids=['missing', 'shape', 'dtype', 'device'])
def test_update_validation(change, match):
    import torch
    result = {'obs': torch.zeros(4, 3, 5), 'actions': torch.zeros(4, 3, 2),
              'values': torch.zeros(4, 3), 'neglogps': torch.zeros(4, 3),
              'rewards': torch.zeros(4, 3), 'dones': torch.zeros(4, 3, dtype=torch.uint8),
              'last_values': torch.zeros(3)}
    change(result, torch)
    with pytest.raises(ValueError, match=match):
        _learner().update(result, noptepochs=1, nminibatches=2)
    with pytest.raises(ValueError, match='do not split'):
        _learner().update(dict(result, actions=torch.zeros(4, 3, 2)), nminibatches=5)


# ------------------------------------------------------ 6. per-call rates
BAD_RATES = [0.0, -1.0, -2.5e-4, float('nan'), float('inf'), 'fast']


def _cpu_result():
    import torch
    return {'obs': torch.zeros(4, 3, 5), 'actions': torch.zeros(4, 3, 2),
            'values': torch.zeros(4, 3), 'neglogps': torch.zeros(4, 3),
            'rewards': torch.zeros(4, 3), 'dones': torch.zeros(4, 3, dtype=torch.uint8),
            'last_values': torch.zeros(3)}


@pytest.mark.parametrize('name', ['lr', 'cliprange'])
@pytest.mark.parametrize('rate', BAD_RATES)
def test_a_per_call_rate_that_is_not_positive_is_refused(name, rate):
    """The native side reads every lr / cliprange that is not positive as
    "none given" (Python sends -1 for None), so a schedule's 0.0 would train
    at the learner's own rate: refused before anything else is looked at."""
    import torch
    learner = _learner()
    kw = {name: rate}
    calls = [lambda: learner.step(_cpu_batch(), **kw),
             lambda: learner.step({}, **kw),                          # before the batch is looked at
             lambda: learner.update(_cpu_result(), nminibatches=2, **kw),
             lambda: learner.update({}, **kw)]
    if name == 'lr':
        records = torch.zeros(1, learner.record_doubles, dtype=torch.float64)
        calls += [lambda: learner.apply(records, 6, lr=rate), lambda: learner.apply(None, 0, lr=rate)]
    else:
        calls += [lambda: learner.grad(_cpu_batch(), cliprange=rate),
                  lambda: learner.partial(_cpu_batch(), cliprange=rate)]
    for call in calls:
        with pytest.raises(ValueError, match='%s must be None or a finite positive number' % name):
            call()


@pytest.mark.parametrize('rate', [None, 1e-30, 2.5e-4, np.float32(0.1), 3])
def test_a_positive_per_call_rate_passes_the_check(rate):
    """The call goes on to the next check, the tensors' device."""
    for call in (lambda: _learner().step(_cpu_batch(), lr=rate, cliprange=rate),
                 lambda: _learner().update(_cpu_result(), nminibatches=2, lr=rate, cliprange=rate),
                 lambda: _learner().grad(_cpu_batch(), cliprange=rate)):
        with pytest.raises(ValueError, match='must be on device cuda:0'):
            call()


# ------------------------------------------------- 7. whole updates' inputs
@pytest.mark.parametrize('call', sorted(cases.UPDATE_CALLS))
@pytest.mark.parametrize('case', cases.UPDATE_CASES, ids=cases.UPDATE_CASE_IDS)
def test_update_draws_stay_off_the_kinks_and_clip(case, call):
    """What test_gpu_ppo2.py's section 8 needs of its committed draws, from
    the statements alone (``cases.update_input_holds``: off the kinks, a step
    that clips, a float32 NumPy trajectory within ``cases.F32_ROOM`` of the
    float64 one); and the committed seed is the first that meets it."""
    rollout, hp, lr, ref = cases.update_reference(case, call)
    ref32 = cases.update_reference(case, call, dtype=np.float32)[3]
    margin, clipfrac, room = cases.update_input_holds(rollout, hp, ref, ref32)
    print(case, call, 'smallest margin %.3g, largest clipfrac %.2f, float32 statement %.3g'
          % (margin, clipfrac, room))
    for seed in range(cases.UPDATE_SEEDS[case, call]):
        earlier = cases.update_reference(case, call, seed=seed)
        with pytest.raises(AssertionError):
            cases.update_input_holds(earlier[0], hp, earlier[3],
                                     cases.update_reference(case, call, np.float32, seed)[3])
    K, R, _, _, _, nminibatches = case
    assert len(ref['stats']) == cases.UPDATE_EPOCHS * nminibatches
    assert ref['returns'].shape == (K, R) and ref['params'].dtype == np.float64
    for perm in rollout['perms']:
        assert sorted(perm) == list(range(K * R))
    # the old policy is the current one: the first step's ratio is 1
    assert float(ref['stats'][0]['approxkl']) < 1e-12 and float(ref['stats'][0]['clipfrac']) == 0.0
    assert all(ref32[n].dtype == np.float32 for n in ('params', 'm', 'v', 'returns'))
    assert pc_rel(ref32['params'], ref['params']) < 1e-5


def pc_rel(got, ref):
    return float(np.max(np.abs(got.astype(np.float64) - ref)) / np.max(np.abs(ref)))
