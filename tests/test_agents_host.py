"""``custom_envs_amd.agents``: the constructors' and ``learn``'s argument
checks, the schedules' arithmetic and the save / load round trip, on
shape-only models (``EnvSpec`` with no device).  No test here needs a GPU."""
import io

import numpy as np
import pytest

from custom_envs_amd import agents
from custom_envs_amd.agents import A2C, PPO2, EnvSpec, MlpPolicy

ARCH = {'net_arch': [dict(pi=[32, 32], vf=[32, 32])]}


def _spec(rows=6):
    return EnvSpec(rows, 9, 4, low=-1.0, high=2.0)


def test_policy_kwargs_map_to_hidden():
    assert agents.hidden_from_policy_kwargs(None) == (64, 64)
    assert agents.hidden_from_policy_kwargs(ARCH) == (32, 32)
    assert PPO2(MlpPolicy, _spec(), n_steps=2, nminibatches=2, policy_kwargs=ARCH).hidden == (32, 32)
    with pytest.raises(ValueError, match='equal widths'):
        A2C(MlpPolicy, _spec(), policy_kwargs={'net_arch': [dict(pi=[64, 64], vf=[64, 32])]})
    with pytest.raises(ValueError, match='equal widths'):
        PPO2(MlpPolicy, _spec(), policy_kwargs={'net_arch': [dict(pi=[64], vf=[64, 64])]})
    with pytest.raises(ValueError, match='net_arch'):
        A2C(MlpPolicy, _spec(), policy_kwargs={'net_arch': [64, 64]})
    with pytest.raises(ValueError, match='net_arch only'):
        A2C(MlpPolicy, _spec(), policy_kwargs={'act_fun': None})


def test_unknown_schedule_and_policy_are_refused():
    with pytest.raises(ValueError, match='lr_schedule'):
        A2C(MlpPolicy, _spec(), lr_schedule='double_linear_con')
    with pytest.raises(ValueError, match='MlpPolicy'):
        A2C('MlpLstmPolicy', _spec())
    with pytest.raises(ValueError, match='cliprange_vf'):
        PPO2(MlpPolicy, _spec(), n_steps=2, nminibatches=2, cliprange=lambda f: 0.2 * f)
    A2C('MlpPolicy', _spec(), lr_schedule='linear')


def test_a_non_engine_env_is_a_type_error():
    for env in (object(), None, [1, 2], 'Optimize-v0'):
        with pytest.raises(TypeError, match='GPUVecEnv or an engine-backed OptVecEnv'):
            PPO2(MlpPolicy, env)
        with pytest.raises(TypeError, match='GPUVecEnv or an engine-backed OptVecEnv'):
            A2C(MlpPolicy, env)


def test_learn_argument_checks():
    model = PPO2(MlpPolicy, _spec(6), n_steps=4, nminibatches=4, policy_kwargs=ARCH)
    assert model.n_batch == 24
    with pytest.raises(ValueError, match='less than one batch'):
        model.learn(23)
    assert model.check_learn(24) == 1 and model.check_learn(71) == 2 and model.check_learn(72) == 3
    with pytest.raises(RuntimeError, match='needs an env'):
        model.learn(48)           # the arguments are fine; there is no env
    with pytest.raises(ValueError, match='do not split into 4 minibatches'):
        PPO2(MlpPolicy, _spec(7), n_steps=3, nminibatches=4, policy_kwargs=ARCH)
    a2c = A2C(MlpPolicy, _spec(6), policy_kwargs=ARCH)
    assert a2c.n_batch == 30
    with pytest.raises(ValueError, match='less than one batch'):
        a2c.learn(29)


def test_schedule_arithmetic():
    assert [agents.ppo2_frac(u, 4) for u in (1, 2, 3, 4)] == [1.0, 0.75, 0.5, 0.25]
    # SB's Scheduler is stepped once per batch row: the value an update uses
    # is the one of its last row, n = u * n_batch - 1
    lr, nb, total = 7e-4, 40, 120
    for u in (1, 2, 3):
        assert agents.linear_schedule_lr(lr, u, nb, total) == lr * (1.0 - (u * nb - 1) / total)
    assert agents.linear_schedule_lr(lr, 3, nb, total) == pytest.approx(lr / total)
    model = A2C(MlpPolicy, _spec(8), learning_rate=lr, lr_schedule='linear', policy_kwargs=ARCH)
    assert model.n_batch == 40
    assert model.lr_at(2, 120) == agents.linear_schedule_lr(lr, 2, 40, 120)
    assert A2C(MlpPolicy, _spec(8), learning_rate=lr, policy_kwargs=ARCH).lr_at(2, 120) == lr
    ppo = PPO2(MlpPolicy, _spec(8), n_steps=2, learning_rate=lambda f: 1e-3 * f, policy_kwargs=ARCH)
    assert ppo.learning_rate(0.5) == 5e-4 and ppo.cliprange(0.5) == 0.2


def test_initial_parameters_are_a_function_of_the_seed():
    a = PPO2(MlpPolicy, _spec(), n_steps=2, nminibatches=2, seed=3, policy_kwargs=ARCH)
    b = PPO2(MlpPolicy, _spec(), n_steps=2, nminibatches=2, seed=3, policy_kwargs=ARCH)
    c = PPO2(MlpPolicy, _spec(), n_steps=2, nminibatches=2, seed=4, policy_kwargs=ARCH)
    assert np.array_equal(a.get_parameters(), b.get_parameters())
    assert not np.array_equal(a.get_parameters(), c.get_parameters())
    layout = a.policy.params_layout()
    flat = a.get_parameters()
    off, shape = layout['pi/w1']
    w = flat[off:off + 32 * 32].reshape(shape).astype(np.float64)
    assert np.allclose(w.T @ w, 2.0 * np.eye(32), atol=1e-5)       # orthogonal, gain sqrt 2
    off, shape = layout['logstd']
    assert np.all(flat[off:] == 0.0)


@pytest.mark.parametrize('cls,kw', [(PPO2, dict(n_steps=2, nminibatches=2, cliprange=0.1)),
                                    (A2C, dict(lr_schedule='linear', alpha=0.9))])
@pytest.mark.parametrize('through', ['path', 'file'])
def test_save_load_round_trip(cls, kw, through, tmp_path):
    model = cls(MlpPolicy, _spec(), seed=2 ** 40 + 7, policy_kwargs=ARCH, **kw)
    rs = np.random.RandomState(0)
    n = model.policy.n_params
    model.set_parameters(rs.normal(0, 1, n).astype(np.float32))
    names = model.learner.OPT_BLOCKS
    opt = {names[0]: rs.uniform(0, 1, n).astype(np.float32),
           names[1]: rs.uniform(0, 1, n).astype(np.float32), 'step': 17 if cls is PPO2 else 0}
    model.set_opt_state(opt)
    model.num_timesteps = 960
    model.rng.advance(33)
    model.rng.epoch, model.rng.predict_t = 5, 2
    if through == 'path':
        target = str(tmp_path / 'model')
        model.save(target)
        source = target                                   # the suffix is added on both sides
        raw = np.load(target + '.npz', allow_pickle=False)
    else:
        target = io.BytesIO()
        model.save(target)
        raw = np.load(io.BytesIO(target.getvalue()), allow_pickle=False)
        source = io.BytesIO(target.getvalue())
    # nothing in the file needs pickle
    assert all(raw[k].dtype != object for k in raw.files)
    assert {'meta', 'params', 'opt_step', 'num_timesteps', 'rng'} <= set(raw.files)
    back = cls.load(source, device=None)
    assert type(back) is cls and back.env is None
    assert np.array_equal(back.get_parameters(), model.get_parameters())
    got = back.get_opt_state()
    assert got['step'] == opt['step']
    for name in names:
        assert np.array_equal(got[name], opt[name])
    assert back.num_timesteps == 960
    assert back.rng.state() == model.rng.state()
    assert back.seed == model.seed and back.hidden == (32, 32)
    for key, value in kw.items():
        assert back.kwargs[key] == value
    assert (back.spec.rows, back.spec.obs_dim, back.spec.act_dim) == (6, 9, 4)
    assert np.array_equal(back.spec.low, model.spec.low)
    with pytest.raises(RuntimeError, match='needs an env'):
        back.learn(10 ** 4)
    other = A2C if cls is PPO2 else PPO2
    with pytest.raises(ValueError, match='holds a'):
        other.load(target + '.npz' if through == 'path' else io.BytesIO(target.getvalue()),
                   device=None)
    # an override replaces a constructor argument
    again = cls.load(target + '.npz' if through == 'path' else io.BytesIO(target.getvalue()),
                     device=None, gamma=0.5)
    assert again.kwargs['gamma'] == 0.5


def test_callable_rates_are_not_stored():
    model = PPO2(MlpPolicy, _spec(), n_steps=2, nminibatches=2, learning_rate=lambda f: 1e-3 * f,
                 policy_kwargs=ARCH)
    buf = io.BytesIO()
    model.save(buf)
    with pytest.raises(ValueError, match='learning_rate was a callable'):
        PPO2.load(io.BytesIO(buf.getvalue()), device=None)
    back = PPO2.load(io.BytesIO(buf.getvalue()), device=None, learning_rate=3e-4)
    assert back.learning_rate(0.3) == 3e-4


def test_opt_state_is_validated_before_c():
    model = PPO2(MlpPolicy, _spec(), n_steps=2, nminibatches=2, policy_kwargs=ARCH)
    n = model.policy.n_params
    good = {'m': np.zeros(n, np.float32), 'v': np.zeros(n, np.float32), 'step': 0}
    model.learner.check_opt_state(good)
    for bad, match in ((dict(good, m=np.zeros(n, np.float64)), 'float32'),
                       (dict(good, v=np.zeros(n + 1, np.float32)), 'shape'),
                       (dict(good, step=-1), 'negative'),
                       ({'m': good['m'], 'step': 0}, "lacks 'v'"),
                       ({'m': good['m'], 'v': good['v']}, "lacks 'step'")):
        with pytest.raises(ValueError, match=match):
            model.learner.check_opt_state(bad)


def test_perms_are_validated():
    torch = pytest.importorskip('torch')
    model = PPO2(MlpPolicy, _spec(), n_steps=2, nminibatches=2, policy_kwargs=ARCH)
    ok = [torch.arange(12, dtype=torch.int32), torch.arange(12, dtype=torch.int32)]
    assert len(model.learner.check_perms(ok, 2, 12)) == 2
    with pytest.raises(ValueError, match='noptepochs'):
        model.learner.check_perms(ok[:1], 2, 12)
    with pytest.raises(ValueError, match='int32'):
        model.learner.check_perms([ok[0], ok[1].long()], 2, 12)
    with pytest.raises(ValueError, match='shape'):
        model.learner.check_perms([ok[0], ok[1][:11]], 2, 12)
