"""The DDPG learner's host side (custom_envs_amd/ddpg.py, the argument checks
of ce_ddpg_* and of collect_ddpg).  Needs the built library, no GPU.

1. The layout: offsets, ``n_params`` and the C count at every case (CASES
   and SHAPE_CASES); the rejected shapes.
2. ``loss_grad_numpy`` in float64 against central differences of the two
   losses (cases 1-4 and SHAPE_CASES): each block within 1e-6 of the largest entry of that
   network's gradient; the actor's loss moves no critic parameter's gradient
   and ``y`` does not move with the online parameters.
3. ``train_step_numpy``: the targets after a step are ``soft_update_numpy`` of
   the new parameters; the two blocks take their own learning rates;
   ``set_params`` makes the targets equal to the parameters.
4. Every validation error of ``act``, ``grad``, ``step``, ``ReplayMemory`` and
   ``collect_ddpg`` without a device, and the C entry points' own checks.
"""
import ctypes

import numpy as np
import pytest
import torch

import ddpg_cases as cases
from custom_envs_amd import _native, ddpg
from custom_envs_amd.ddpg import DDPGAgent, ReplayMemory
from custom_envs_amd.policy import flat_to_dict
from custom_envs_amd.ppo2 import adam_step_numpy
from custom_envs_amd.vectorize.collect import check_collect_ddpg


# ------------------------------------------------------------------- 1. layout
@pytest.mark.parametrize('case', cases.CASES + cases.SHAPE_CASES, ids=str)
def test_layout_and_n_params(case):
    _, D, hidden, A, _ = case
    layout = ddpg.params_layout(D, A, hidden)
    names = list(layout)
    L = len(hidden)
    assert names[:2] == ['actor/w0', 'actor/b0'] and names[-2:] == ['critic/w_out', 'critic/b_out']
    assert len(names) == 4 * (L + 1)
    off = 0
    for name, (o, shape) in layout.items():       # contiguous, in order
        assert o == off, name
        off += int(np.prod(shape))
    assert layout['actor/w0'][1] == (D, hidden[0]) and layout['critic/w0'][1] == (D, hidden[0])
    assert layout['actor/w_out'][1] == (hidden[-1], A)
    concat = 'critic/w1' if L == 2 else 'critic/w_out'       # the + A rows
    assert layout[concat][1][0] == hidden[0] + A
    if L == 2:
        assert layout['actor/w1'][1] == (hidden[0], hidden[1])
        assert layout['critic/w_out'][1] == (hidden[1], 1)
    assert layout['critic/w_out'][1][1] == 1 and layout['critic/b_out'][1] == (1,)
    agent = DDPGAgent(D, A, hidden, device=None)
    assert agent.n_params == off == ddpg.n_params(D, A, hidden)
    assert agent.n_actor == layout['critic/w0'][0] == ddpg.n_actor_params(D, A, hidden)
    assert ddpg._act_dim_of(off, D, hidden) == A


def test_shape_cases_leave_the_draws_of_cases_alone():
    """``draw_case`` seeds from the position in CASES + SHAPE_CASES."""
    both = cases.CASES + cases.SHAPE_CASES
    assert len(set(both)) == len(both)
    assert [both.index(c) for c in cases.CASES] == list(range(len(cases.CASES)))
    for case in cases.SHAPE_CASES:
        inp = cases.draw_case(case)          # asserts its own margins and shares
        assert inp['obs0'].shape == (case[0], case[1]) and inp['redraws'] >= 1


@pytest.mark.parametrize('D, A, hidden', [(5, 2, (16,)), (5, 2, (96,)), (5, 2, (128,)),
                                          (5, 2, (64, 128)), (5, 2, ()), (5, 2, (32, 32, 32)),
                                          (129, 2, (32,)), (5, 65, (32,))])
def test_unsupported_shapes_are_loud(D, A, hidden):
    with pytest.raises(_native.NativeEngineError):
        DDPGAgent(D, A, hidden, device=None)


def test_c_shape_limits():
    lib = _native.load()

    def n(D=5, A=2, hidden=(32,), abi=_native.ABI_VERSION):
        cfg = _native.CeDdpgConfig(abi_version=abi, obs_dim=D, act_dim=A, n_hidden=len(hidden))
        for i, h in enumerate(hidden):
            cfg.hidden[i] = h
        return lib.ce_ddpg_n_params(ctypes.byref(cfg))

    assert n() == ddpg.n_params(5, 2, (32,))
    assert n(128, 64, (64, 64)) == ddpg.n_params(128, 64, (64, 64))
    for bad in (dict(hidden=(16,)), dict(hidden=(96,)), dict(hidden=(128,)), dict(hidden=()),
                dict(hidden=(32, 32, 32)), dict(D=129), dict(A=65)):
        assert n(**bad) == _native.CE_EUNSUPPORTED, bad
    assert n(abi=999) == _native.CE_EINVAL
    assert n(D=0) == _native.CE_EINVAL
    assert lib.ce_ddpg_n_params(None) == _native.CE_EINVAL


def test_init_params_numpy():
    D, A, hidden = 15, 3, (64, 32)
    flat = ddpg.init_params_numpy(D, A, hidden, seed=3)
    assert flat.dtype == np.float32 and flat.shape == (ddpg.n_params(D, A, hidden),)
    p = flat_to_dict(flat, ddpg.params_layout(D, A, hidden))
    for name, value in p.items():
        if value.ndim == 1:
            assert not value.any(), name
        elif name.endswith('w_out'):
            assert np.abs(value).max() <= 3e-3 and value.std() > 1e-3, name
        else:
            limit = np.sqrt(6.0 / sum(value.shape))
            assert np.abs(value).max() <= limit and value.std() > 0.4 * limit, name
    assert np.array_equal(flat, ddpg.init_params_numpy(D, A, hidden, seed=3))
    assert not np.array_equal(flat, ddpg.init_params_numpy(D, A, hidden, seed=4))


# ----------------------------------------------- 2. the gradient's correctness
def _losses(flat, inp):
    """(critic_loss, actor_loss) of the float64 statement's forward parts."""
    hidden = inp['hidden']
    y = ddpg.target_numpy(inp['target_params'], inp['rewards'], inp['obs1'], inp['dones'],
                          cases.HP.gamma, hidden)
    q = ddpg.critic_numpy(flat, inp['obs0'], inp['actions'], hidden)
    a = ddpg.actor_numpy(flat, inp['obs0'], hidden=hidden)
    qa = ddpg.critic_numpy(flat, inp['obs0'], a, hidden)
    return np.mean((q - y) ** 2), -np.mean(qa)


@pytest.mark.parametrize('case', cases.CASES[:4] + cases.SHAPE_CASES, ids=str)
def test_loss_grad_against_central_differences(case):
    inp = cases.draw_case(case)
    _, D, hidden, A, _ = case
    stats, grad = cases.reference(case)
    flat = inp['params'].astype(np.float64)
    layout = ddpg.params_layout(D, A, hidden)
    n_actor = layout['critic/w0'][0]
    crit, act = _losses(flat, inp)
    assert abs(crit - stats['critic_loss']) <= 1e-12 * abs(crit)
    assert abs(act - stats['actor_loss']) <= 1e-12 * abs(act)
    h = 1e-5
    rs = np.random.RandomState(0)
    scale = {'actor': np.abs(grad[:n_actor]).max(), 'critic': np.abs(grad[n_actor:]).max()}
    for name, (off, shape) in layout.items():
        size = int(np.prod(shape))
        picks = np.arange(size) if size <= 12 else rs.choice(size, 12, replace=False)
        net = name.split('/')[0]
        for i in off + picks:
            up, dn = flat.copy(), flat.copy()
            up[i] += h
            dn[i] -= h
            (cu, au), (cd, ad) = _losses(up, inp), _losses(dn, inp)
            if net == 'critic':
                fd = (cu - cd) / (2 * h)
            else:
                fd = (au - ad) / (2 * h)
                assert cu == cd          # the critic's loss does not see the actor
            assert abs(fd - grad[i]) <= 1e-6 * scale[net], (name, i, fd, grad[i])
    # the actor's loss has a gradient on the critic's parameters; none of it is
    # in the critic's block, which is d critic_loss alone
    i = layout['critic/b_out'][0]
    up, dn = flat.copy(), flat.copy()
    up[i] += h
    dn[i] -= h
    assert abs((_losses(up, inp)[1] - _losses(dn, inp)[1]) / (2 * h) + 1.0) < 1e-6
    assert abs(grad[i] - 2 * (stats['q_mean'] - stats['target_mean'])) <= 1e-12 * scale['critic']


@pytest.mark.parametrize('case', cases.CASES[:4], ids=str)
def test_actor_gradient_alone_leaves_critic_block_zero(case):
    """With the critic's loss at its minimum (y = Q) the critic's block is the
    critic's loss gradient alone: exactly zero, whatever the actor's loss does."""
    inp = cases.draw_case(case)
    hidden = inp['hidden']
    q = ddpg.critic_numpy(inp['params'], inp['obs0'], inp['actions'], hidden)
    n_actor = ddpg.n_actor_params(case[1], case[3], hidden)
    # rewards = Q and every row done: y = Q exactly
    stats, grad = ddpg.loss_grad_numpy(inp['params'], inp['target_params'], inp['obs0'],
                                       inp['actions'], q, inp['obs1'], np.ones(case[0], np.uint8),
                                       hp=cases.HP, hidden=hidden)
    assert stats['critic_loss'] == 0.0 and not grad[n_actor:].any()
    assert np.abs(grad[:n_actor]).max() > 0


def test_target_is_constant_in_the_online_parameters():
    inp = cases.draw_case(cases.CASES[2])
    hidden = inp['hidden']
    y = ddpg.target_numpy(inp['target_params'], inp['rewards'], inp['obs1'], inp['dones'],
                          cases.HP.gamma, hidden)
    done = inp['dones'] != 0
    assert done.any() and not done.all()
    assert np.array_equal(y[done], inp['rewards'][done].astype(np.float64))
    other = inp['params'] + 1.0
    s0, _ = ddpg.loss_grad_numpy(inp['params'], inp['target_params'], *[inp[n] for n in cases.FIELDS],
                                 hp=cases.HP, hidden=hidden)
    s1, _ = ddpg.loss_grad_numpy(other, inp['target_params'], *[inp[n] for n in cases.FIELDS],
                                 hp=cases.HP, hidden=hidden)
    assert s0['target_mean'] == s1['target_mean'] == np.mean(y)
    assert s0['q_mean'] != s1['q_mean']


def test_statement_clips_observations_and_noise():
    inp = cases.draw_case(cases.CASES[1])
    hidden = inp['hidden']
    clipped = np.clip(inp['obs0'], -5, 5)
    assert not np.array_equal(clipped, inp['obs0'])
    a = ddpg.actor_numpy(inp['params'], inp['obs0'], hidden=hidden)
    assert np.array_equal(a, ddpg.actor_numpy(inp['params'], clipped, hidden=hidden))
    assert np.abs(a).max() <= 1.0
    noise = np.full(a.shape, 3.0)
    assert np.array_equal(ddpg.actor_numpy(inp['params'], inp['obs0'], noise, hidden), np.ones_like(a))
    q = ddpg.critic_numpy(inp['params'], inp['obs0'], inp['actions'], hidden)
    assert q.shape == (case_rows(inp),)
    assert np.array_equal(q, ddpg.critic_numpy(inp['params'], clipped, inp['actions'], hidden))
    # the dict form and the flat form agree
    as_dict = flat_to_dict(inp['params'], ddpg.params_layout(5, 2, hidden))
    assert np.array_equal(a, ddpg.actor_numpy(as_dict, inp['obs0'], hidden=hidden))


def case_rows(inp):
    return inp['obs0'].shape[0]


# ------------------------------------------------------------- 3. the train step
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_train_step_numpy(dtype):
    case = cases.CASES[3]
    inp = cases.draw_case(case)
    hidden = inp['hidden']
    n_actor = ddpg.n_actor_params(case[1], case[3], hidden)
    p0, t0 = inp['params'].astype(dtype), inp['target_params'].astype(dtype)
    m0, v0 = np.zeros_like(p0), np.zeros_like(p0)
    batch = cases.batch_of(inp)
    kw = dict(hp=cases.HP, hidden=hidden, tau=0.01, actor_lr=1e-4, critic_lr=1e-3)
    p1, t1, m1, v1, stats = ddpg.train_step_numpy(p0, t0, m0, v0, 1, batch, n_actor, **kw)
    assert all(a.dtype == dtype for a in (p1, t1, m1, v1))
    assert np.array_equal(t1, ddpg.soft_update_numpy(t0, p1, 0.01))
    assert np.array_equal(t1, dtype(1 - 0.01) * t0 + dtype(0.01) * p1)
    _, grad = ddpg.loss_grad_numpy(p0, t0, *[inp[n] for n in cases.FIELDS], hp=cases.HP,
                                   hidden=hidden, dtype=dtype)
    for block, lr in ((slice(0, n_actor), 1e-4), (slice(n_actor, None), 1e-3)):
        ref = adam_step_numpy(p0[block], grad[block], m0[block], v0[block], 1, lr,
                              max_grad_norm=0, eps=1e-8)
        assert np.array_equal(p1[block], ref[0]) and np.array_equal(m1[block], ref[1])
        assert np.array_equal(v1[block], ref[2])
    # the first Adam step moves every parameter with a gradient by its block's lr
    moved = np.abs(p1 - p0)
    live = np.abs(grad) > 1e-3 * np.abs(grad).max()
    assert np.allclose(moved[:n_actor][live[:n_actor]], 1e-4, rtol=1e-3)
    assert np.allclose(moved[n_actor:][live[n_actor:]], 1e-3, rtol=1e-3)
    # a second step shares t = 2 between the blocks
    p2, t2, _, _, _ = ddpg.train_step_numpy(p1, t1, m1, v1, 2, batch, n_actor, **kw)
    assert np.array_equal(t2, ddpg.soft_update_numpy(t1, p2, 0.01))


def test_set_params_copies_into_the_targets():
    case = cases.CASES[3]
    inp = cases.draw_case(case)
    agent = DDPGAgent(case[1], case[3], case[2], device=None)
    with pytest.raises(ValueError, match='no parameters'):
        agent.get_params()
    agent.set_params(inp['params'])
    assert np.array_equal(agent.get_params(), inp['params'])
    assert np.array_equal(agent.get_params(target=True), inp['params'])
    as_dict = flat_to_dict(inp['target_params'], agent.params_layout())
    agent.set_params(as_dict)
    assert np.array_equal(agent.get_params(target=True), inp['target_params'])
    with pytest.raises(ValueError, match='parameters'):
        agent.set_params(inp['params'][:-1])
    with pytest.raises(ValueError, match='float32'):
        agent.set_params(torch.zeros(agent.n_params, dtype=torch.float64))
    with pytest.raises(ValueError, match='shape'):
        agent.set_params(torch.zeros(agent.n_params + 1))


# ------------------------------------------------------ 4. the argument checks
D, A, HID = 15, 2, (64, 32)


def _agent():
    return DDPGAgent(D, A, HID, device=None)


def _batch(m=6):
    return {'obs0': torch.zeros(m, D), 'actions': torch.zeros(m, A), 'rewards': torch.zeros(m),
            'obs1': torch.zeros(m, D), 'dones': torch.zeros(m, dtype=torch.uint8)}


def test_act_validation():
    agent = _agent()
    assert agent.check_act(torch.zeros(4, D)) == 4
    assert agent.check_act(torch.zeros(4, D), torch.zeros(4, A),
                           {'action': torch.zeros(4, A), 'env_action': torch.zeros(4, A)}) == 4
    with pytest.raises(ValueError, match='obs must have dtype float32'):
        agent.check_act(torch.zeros(4, D, dtype=torch.float64))
    with pytest.raises(ValueError, match='obs must have shape'):
        agent.check_act(torch.zeros(4, D + 1))
    with pytest.raises(ValueError, match='obs must have shape'):
        agent.check_act(torch.zeros(4 * D))
    with pytest.raises(ValueError, match='obs must be contiguous'):
        agent.check_act(torch.zeros(D, 4).t())
    with pytest.raises(ValueError, match='noise must have shape'):
        agent.check_act(torch.zeros(4, D), torch.zeros(3, A))
    with pytest.raises(ValueError, match='noise must have dtype'):
        agent.check_act(torch.zeros(4, D), torch.zeros(4, A, dtype=torch.float16))
    with pytest.raises(ValueError, match='noise must be contiguous'):
        agent.check_act(torch.zeros(4, D), torch.zeros(4, 2 * A)[:, ::2])
    with pytest.raises(ValueError, match="lack 'env_action'"):
        agent.check_act(torch.zeros(4, D), None, {'action': torch.zeros(4, A)})
    with pytest.raises(ValueError, match='act output action must have shape'):
        agent.check_act(torch.zeros(4, D), None,
                        {'action': torch.zeros(5, A), 'env_action': torch.zeros(4, A)})
    with pytest.raises(ValueError, match='act output env_action must be contiguous'):
        agent.check_act(torch.zeros(4, D), None,
                        {'action': torch.zeros(4, A), 'env_action': torch.zeros(A, 4).t()})


def test_batch_validation():
    agent = _agent()
    assert agent.check_batch(_batch()) == (6, 6)
    assert agent.check_batch(_batch(), torch.zeros(9, dtype=torch.int32)) == (6, 9)
    for name in cases.FIELDS:
        b = _batch()
        del b[name]
        with pytest.raises(ValueError, match='batch lacks %r' % name):
            agent.check_batch(b)
    b = _batch()
    b['obs0'] = torch.zeros(6 * D)
    with pytest.raises(ValueError, match=r'obs0 must have shape \[M\]'):
        agent.check_batch(b)
    b = _batch()
    b['obs0'] = torch.zeros(6, D, dtype=torch.float64)
    with pytest.raises(ValueError, match='obs0 must have dtype float32'):
        agent.check_batch(b)
    b = _batch()
    b['obs1'] = torch.zeros(6, D + 1)
    with pytest.raises(ValueError, match='obs1 must have shape'):
        agent.check_batch(b)
    b = _batch()
    b['actions'] = torch.zeros(6, A + 1)
    with pytest.raises(ValueError, match='actions must have shape'):
        agent.check_batch(b)
    b = _batch()
    b['rewards'] = torch.zeros(12)[::2]
    with pytest.raises(ValueError, match='rewards must be contiguous'):
        agent.check_batch(b)
    b = _batch()
    b['dones'] = torch.zeros(6, dtype=torch.bool)
    with pytest.raises(ValueError, match='dones must have dtype uint8'):
        agent.check_batch(b)
    b = _batch()
    b['dones'] = torch.zeros(5, dtype=torch.uint8)
    with pytest.raises(ValueError, match='dones must have shape'):
        agent.check_batch(b)
    with pytest.raises(ValueError, match='idx must have dtype int32'):
        agent.check_batch(_batch(), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match='idx must have shape'):
        agent.check_batch(_batch(), torch.zeros((2, 2), dtype=torch.int32))
    with pytest.raises(ValueError, match='idx must be contiguous'):
        agent.check_batch(_batch(), torch.zeros(8, dtype=torch.int32)[::2])
    # a per-call rate: None is the agent's, 0 freezes, anything below is refused
    assert agent._rate('actor_lr', None) == -1.0 and agent._rate('actor_lr', 0) == 0.0
    for bad in (-1e-4, float('nan')):
        with pytest.raises(ValueError, match='critic_lr must be >= 0'):
            agent.step(_batch(), critic_lr=bad)
    # grad / step / target validate first, then refuse to run without a device
    for call in (agent.grad, agent.step, agent.target):
        with pytest.raises(ValueError, match='idx must have dtype int32'):
            call(_batch(), torch.zeros(4, dtype=torch.int64))
        with pytest.raises(_native.NativeEngineError, match='shape-only'):
            call(_batch())


def test_replay_memory_validation_and_ring():
    with pytest.raises(ValueError, match='multiple of rows'):
        ReplayMemory(10, 3, D, A, device=None)
    with pytest.raises(ValueError, match='multiple of rows'):
        ReplayMemory(2, 3, D, A, device=None)
    with pytest.raises(ValueError, match='rows must be'):
        ReplayMemory(4, 0, D, A, device=None)
    mem = ReplayMemory(12, 3, D, A, device=None)
    assert (mem.size, mem.pos) == (0, 0)
    with pytest.raises(ValueError, match='empty'):
        mem.sample(4)
    batch = mem.as_batch()
    assert tuple(batch) == cases.FIELDS
    assert batch['obs0'].shape == (12, D) and batch['dones'].dtype == torch.uint8
    assert _agent().check_batch(batch) == (12, 12)
    for step in range(5):
        assert mem.slot() == slice(3 * (step % 4), 3 * (step % 4) + 3)
        mem.obs0[mem.slot()] = float(step)          # a contiguous slice of the field
        assert mem.obs0[mem.slot()].is_contiguous()
        mem.advance()
        assert mem.size == min(3 * (step + 1), 12)
    assert (mem.size, mem.pos) == (12, 3)
    assert mem.obs0[0, 0] == 4.0 and mem.obs0[3, 0] == 1.0      # the ring wrapped
    gen = torch.Generator().manual_seed(5)
    idx = mem.sample(64, generator=gen)
    assert idx.dtype == torch.int32 and idx.shape == (64,)
    assert int(idx.min()) >= 0 and int(idx.max()) < 12
    assert torch.equal(idx, mem.sample(64, generator=torch.Generator().manual_seed(5)))
    with pytest.raises(ValueError, match='n must be'):
        mem.sample(0)
    part = ReplayMemory(12, 3, D, A, device=None)
    part.advance()
    assert int(part.sample(50).max()) < 3           # only the valid records


def test_collect_ddpg_validation():
    agent, mem = _agent(), ReplayMemory(12, 3, D, A, device=None)
    assert check_collect_ddpg(agent, mem, 5, None, 3, D, A) == 5
    assert check_collect_ddpg(agent, mem, 2, torch.zeros(2, 3, A), 3, D, A) == 2
    with pytest.raises(TypeError, match='DDPGAgent'):
        check_collect_ddpg(object(), mem, 5, None, 3, D, A)
    with pytest.raises(TypeError, match='ReplayMemory'):
        check_collect_ddpg(agent, {}, 5, None, 3, D, A)
    with pytest.raises(ValueError, match='the agent maps'):
        check_collect_ddpg(agent, mem, 5, None, 3, D + 1, A)
    with pytest.raises(ValueError, match='the memory holds'):
        check_collect_ddpg(agent, ReplayMemory(12, 3, D, A + 1, device=None), 5, None, 3, D, A)
    with pytest.raises(ValueError, match='rows per step'):
        check_collect_ddpg(agent, mem, 5, None, 4, D, A)
    with pytest.raises(ValueError, match='n_steps must be'):
        check_collect_ddpg(agent, mem, 0, None, 3, D, A)
    with pytest.raises(ValueError, match=r'noise must be \[>= k\]'):
        check_collect_ddpg(agent, mem, 5, torch.zeros(4, 3, A), 3, D, A)
    with pytest.raises(ValueError, match=r'noise must be \[>= k\]'):
        check_collect_ddpg(agent, mem, 5, torch.zeros(5, 3 * A), 3, D, A)
    with pytest.raises(ValueError, match='noise must have shape'):
        check_collect_ddpg(agent, mem, 5, torch.zeros(5, 4, A), 3, D, A)
    with pytest.raises(ValueError, match='noise must have dtype'):
        check_collect_ddpg(agent, mem, 5, torch.zeros(5, 3, A, dtype=torch.float64), 3, D, A)
    with pytest.raises(ValueError, match='noise must be contiguous'):
        check_collect_ddpg(agent, mem, 5, torch.zeros(5, 3, 2 * A)[:, :, ::2], 3, D, A)


def test_host_path_optvecenv_has_no_collect_ddpg():
    from custom_envs_amd.vectorize.optvecenv import OptVecEnv
    env = OptVecEnv.__new__(OptVecEnv)
    env._engine = None
    with pytest.raises(NotImplementedError, match='engine-backed'):
        env.collect_ddpg(_agent(), None, 1)


# -------------------------------------------------------- the C entry points
def _cfg(**over):
    base = dict(abi_version=_native.ABI_VERSION, device=0, obs_dim=D, act_dim=A, n_hidden=2,
                grid_limit=0, gamma=0.99, tau=0.001, actor_lr=1e-4, critic_lr=1e-3, beta1=0.9,
                beta2=0.999, eps=1e-8, obs_lo=-5.0, obs_hi=5.0)
    base.update(over)
    cfg = _native.CeDdpgConfig(**base)
    cfg.hidden[0], cfg.hidden[1] = HID
    return cfg


def _refused(rc, word):
    msg = _native.load().ce_last_error().decode()
    assert rc == _native.CE_EINVAL, (rc, msg)
    assert word in msg, msg


def test_new_symbols_are_exported():
    lib = _native.load()
    for name in ('ce_ddpg_n_params', 'ce_ddpg_create', 'ce_ddpg_destroy', 'ce_ddpg_set_params',
                 'ce_ddpg_get_params', 'ce_ddpg_act', 'ce_ddpg_target', 'ce_ddpg_grad',
                 'ce_ddpg_step'):
        assert name in _native.EXPORTS and hasattr(lib, name), name
    assert lib.ce_abi_version() == 5
    assert ctypes.sizeof(_native.CeDdpgConfig) == 10 * 4 + 9 * 8 + 64 * 4


@pytest.mark.parametrize('over, word', [
    (dict(gamma=1.5), 'gamma'), (dict(gamma=float('nan')), 'gamma'), (dict(tau=-0.1), 'tau'),
    (dict(tau=2.0), 'tau'), (dict(actor_lr=0.0), 'actor_lr'), (dict(critic_lr=-1.0), 'critic_lr'),
    (dict(critic_lr=float('nan')), 'critic_lr'), (dict(beta1=1.0), 'beta1'),
    (dict(beta2=-0.5), 'beta2'), (dict(eps=0.0), 'eps'), (dict(obs_lo=5.0), 'obs_lo'),
    (dict(obs_hi=float('nan')), 'obs_lo'), (dict(grid_limit=-1), 'grid_limit')],
    ids=lambda v: None if isinstance(v, str) else '%s=%s' % next(iter(v.items())))
def test_create_refuses_bad_hyperparameters(over, word):
    lib = _native.load()
    handle = ctypes.c_void_p()
    cfg = _cfg(**over)
    _refused(lib.ce_ddpg_create(ctypes.byref(cfg), ctypes.byref(handle)), word)
    assert not handle.value


def test_create_refuses_null_and_infinite_arguments():
    lib = _native.load()
    handle = ctypes.c_void_p()
    cfg = _cfg()
    _refused(lib.ce_ddpg_create(None, ctypes.byref(handle)), 'null config')
    _refused(lib.ce_ddpg_create(ctypes.byref(cfg), None), 'null output')
    cfg.scale[1] = float('inf')
    _refused(lib.ce_ddpg_create(ctypes.byref(cfg), ctypes.byref(handle)), 'scale')
    lib.ce_ddpg_destroy(None)       # a no-op


def test_entry_point_argument_checks():
    lib = _native.load()
    buf = np.zeros(64, np.float32)
    a = buf.ctypes.data

    def act(obs=a, rows=4, action=a, env_action=a):
        return lib.ce_ddpg_act(None, obs, None, rows, action, env_action, None)

    _refused(act(rows=0), 'rows must')
    _refused(act(rows=(1 << 24) + 1), 'rows must')
    _refused(act(obs=None), 'null obs')
    _refused(act(action=None), 'null action')
    _refused(act(env_action=None), 'null env_action')
    _refused(act(), 'null learner')

    def target(n=4, m=8, idx=None, obs1=a, rewards=a, dones=a, y=a):
        return lib.ce_ddpg_target(None, n, m, idx, obs1, rewards, dones, y, None)

    _refused(target(n=0), 'n must')
    _refused(target(m=0), 'm must')
    _refused(target(n=9), 'n exceeds m')
    _refused(target(obs1=None), 'null obs1')
    _refused(target(rewards=None), 'null rewards')
    _refused(target(dones=None), 'null dones')
    _refused(target(y=None), 'null y')
    _refused(target(n=9, idx=a), 'null learner')

    def grad(n=4, m=8, idx=None, obs0=a, actions=a, rewards=a, obs1=a, dones=a, y=a, g=a,
             stats=a):
        return lib.ce_ddpg_grad(None, n, m, idx, obs0, actions, rewards, obs1, dones, y, g, stats,
                                None)

    def step(n=4, m=8, idx=None, obs0=a, actions=a, rewards=a, obs1=a, dones=a, y=a, lr=-1.0,
             stats=a):
        return lib.ce_ddpg_step(None, n, m, idx, obs0, actions, rewards, obs1, dones, y, lr, lr,
                                stats, None)

    for call in (grad, step):
        _refused(call(n=0), 'n must')
        _refused(call(m=(1 << 24) + 1), 'm must')
        _refused(call(n=9), 'n exceeds m')
        _refused(call(obs0=None), 'null obs0')
        _refused(call(actions=None), 'null actions')
        _refused(call(rewards=None), 'null rewards')
        _refused(call(obs1=None), 'null obs1')
        _refused(call(dones=None), 'null dones')
        _refused(call(y=None), 'null y buffer')
        _refused(call(stats=None), 'null stats')
        _refused(call(), 'null learner')
    _refused(grad(g=None), 'null grad')
    _refused(step(lr=float('nan')), 'not a number')
    for name in ('ce_ddpg_set_params', 'ce_ddpg_get_params'):
        _refused(getattr(lib, name)(None, None, 4, 0, None), 'null parameter')
        _refused(getattr(lib, name)(None, a, 4, 0, None), 'null learner')


def test_agent_without_gpu_fails_loudly():
    if torch.cuda.is_available():
        pytest.skip('a GPU is present')
    with pytest.raises(_native.NativeEngineError):
        DDPGAgent(D, A, HID)
