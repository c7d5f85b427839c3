"""The device VecNormalize's C ABI and Python surface without a device: the
exports, every argument check of ``ce_vecnorm_*`` and of the normalised rollout
entries (all of which precede the first HIP call), and the refusals of the
wrapper."""
import ctypes
import functools

import numpy as np
import pytest

from custom_envs_amd import _native
from custom_envs_amd.vectorize import vecnormalize as vnz

EINVAL = _native.CE_EINVAL
NEW = ('ce_vecnorm_create', 'ce_vecnorm_destroy', 'ce_vecnorm_step', 'ce_vecnorm_get_state',
       'ce_vecnorm_set_state', 'ce_rollout_policy_vecnorm', 'ce_multi_rollout_policy_vecnorm')


def _err(lib):
    return lib.ce_last_error().decode()


def test_symbols_are_exported_and_the_abi_version_stays():
    lib = _native.load()
    assert lib.ce_abi_version() == 5 == _native.ABI_VERSION
    for name in NEW:
        assert name in _native.EXPORTS and hasattr(lib, name), name


def _cfg(**change):
    base = dict(abi_version=_native.ABI_VERSION, device=0, rows=4, obs_dim=3, norm_obs=1,
                norm_reward=1, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8)
    base.update(change)
    return _native.CeVecnormConfig(**base)


@pytest.mark.parametrize('change,word', [
    (dict(abi_version=4), 'ABI'), (dict(device=-1), 'device'), (dict(rows=0), 'rows'),
    (dict(rows=-3), 'rows'), (dict(rows=(1 << 24) + 1), 'rows'), (dict(obs_dim=0), 'obs_dim'),
    (dict(obs_dim=(1 << 16) + 1), 'obs_dim'), (dict(clip_obs=0.0), 'clip'),
    (dict(clip_reward=-1.0), 'clip'), (dict(clip_obs=float('nan')), 'clip'),
    (dict(gamma=float('inf')), 'gamma'), (dict(epsilon=-1e-8), 'epsilon'),
    (dict(epsilon=float('nan')), 'epsilon')])
def test_create_checks_its_config_before_any_device_call(change, word):
    lib = _native.load()
    handle = ctypes.c_void_p()
    cfg = _cfg(**change)
    assert lib.ce_vecnorm_create(ctypes.byref(cfg), ctypes.byref(handle)) == EINVAL
    assert word in _err(lib) and not handle.value


def test_create_null_arguments():
    lib = _native.load()
    handle = ctypes.c_void_p()
    cfg = _cfg()
    assert lib.ce_vecnorm_create(None, ctypes.byref(handle)) == EINVAL and 'null' in _err(lib)
    assert lib.ce_vecnorm_create(ctypes.byref(cfg), None) == EINVAL and 'null' in _err(lib)
    assert lib.ce_vecnorm_destroy(None) is None


def test_step_checks():
    lib = _native.load()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    step = lib.ce_vecnorm_step
    # a null handle with everything else valid
    assert step(None, p, p, p, p, p, 1, None) == EINVAL and 'null normaliser' in _err(lib)
    assert step(None, p, None, None, p, None, 2, None) == EINVAL and 'null normaliser' in _err(lib)
    assert step(None, p, None, None, p, None, 4, None) == EINVAL and 'null normaliser' in _err(lib)
    # the plain arguments come first: checked even with a handle given
    fake = p
    assert step(fake, None, p, p, p, p, 1, None) == EINVAL and 'null obs' in _err(lib)
    assert step(fake, p, p, p, None, p, 1, None) == EINVAL and 'null obs' in _err(lib)
    for args in ((p, None, p, p, p), (p, p, None, p, p), (p, p, p, p, None)):
        assert step(fake, *args, 1, None) == EINVAL and 'null reward' in _err(lib)
    assert step(fake, p, p, p, p, p, 8, None) == EINVAL and 'unknown flags' in _err(lib)
    assert step(fake, p, None, None, p, None, 4 | 1, None) == EINVAL and 'OBS_ONLY' in _err(lib)
    assert step(fake, p, None, None, p, None, 4 | 2, None) == EINVAL and 'OBS_ONLY' in _err(lib)
    assert step(fake, p + 2, p, p, p, p, 1, None) == EINVAL and 'aligned' in _err(lib)
    assert step(fake, p, p, p, p, p + 1, 1, None) == EINVAL and 'aligned' in _err(lib)


@pytest.mark.parametrize('name', ['ce_vecnorm_get_state', 'ce_vecnorm_set_state'])
def test_state_checks(name):
    lib = _native.load()
    fn = getattr(lib, name)
    buf = np.zeros(8)
    p = buf.ctypes.data
    assert fn(None, p, p, p, p, p, p, p, None) == EINVAL and 'null normaliser' in _err(lib)
    for i in range(7):
        args = [p] * 7
        args[i] = None
        assert fn(p, *args, None) == EINVAL and 'null' in _err(lib), i


def _rollout_args(multi, **change):
    """Valid plain arguments of a normalised rollout; the three handles are
    dummies, which the plain checks never read."""
    buf = np.zeros(256, np.float32)
    p = buf.ctypes.data + (-buf.ctypes.data % 16)
    out_t = _native.CeMultiOutputs if multi else _native.CeOutputs
    a = dict(eng=p, policy=p, vn=p, k=2, obs_norm=p, obs_step=64, reward_norm=p, reward_step=16,
             flags=1, noise=_native.CeRolloutNoise(), out=out_t(), out_step=256,
             pout=_native.CePolicyOutputs(), pout_step=256)
    a.update(change)
    ref = lambda v: None if v is None else ctypes.byref(v)
    return buf, [a['eng'], a['policy'], a['vn'], a['k'], a['obs_norm'], a['obs_step'],
                 a['reward_norm'], a['reward_step'], a['flags'], ref(a['noise']), ref(a['out']),
                 a['out_step'], ref(a['pout']), a['pout_step']]


@pytest.mark.parametrize('multi', [False, True], ids=['optimize', 'multi'])
@pytest.mark.parametrize('change,word', [
    (dict(eng=None), 'null engine'), (dict(policy=None), 'null policy'),
    (dict(vn=None), 'null normaliser'), (dict(obs_norm=None), 'null normalised'),
    (dict(reward_norm=None), 'null normalised'), (dict(noise=None), 'null noise'),
    (dict(out=None), 'null outputs'), (dict(pout=None), 'null outputs'),
    (dict(k=0), 'k must be positive'), (dict(k=-2), 'k must be positive'),
    (dict(noise=_native.CeRolloutNoise(kind=2)), 'noise kind'),
    (dict(flags=2), 'CE_VECNORM_TRAINING only'), (dict(flags=4), 'CE_VECNORM_TRAINING only'),
    (dict(obs_step=60), 'multiple of 16'), (dict(obs_step=0), 'multiple of 16'),
    (dict(obs_step=-16), 'multiple of 16'), (dict(reward_step=12), 'multiple of 16'),
    (dict(reward_step=0), 'multiple of 16')])
def test_rollout_plain_checks(multi, change, word):
    """Null pointers, k, the noise kind, the flags and the strides: CE_EINVAL
    before any handle is read (so with dummy handles, on a machine without a
    device)."""
    lib = _native.load()
    fn = lib.ce_multi_rollout_policy_vecnorm if multi else lib.ce_rollout_policy_vecnorm
    keep, args = _rollout_args(multi, **change)
    assert fn(*args) == EINVAL
    assert word in _err(lib), _err(lib)
    assert ('ce_multi_rollout' if multi else 'ce_rollout') in _err(lib)


@pytest.mark.parametrize('multi', [False, True], ids=['optimize', 'multi'])
def test_rollout_misaligned_buffers(multi):
    lib = _native.load()
    fn = lib.ce_multi_rollout_policy_vecnorm if multi else lib.ce_rollout_policy_vecnorm
    keep, args = _rollout_args(multi)
    base = args[4]
    args[4] = base + 4
    assert fn(*args) == EINVAL and '16-byte aligned' in _err(lib)
    args[4], args[6] = base, base + 2
    assert fn(*args) == EINVAL and '4-byte aligned' in _err(lib)


# ------------------------------------------------- the Python-side validation
class _Shape:
    """What check_normalized_rollout reads of a DeviceVecNorm."""

    def __init__(self, rows, obs_dim, device=0):
        self.rows, self.obs_dim, self.device = rows, obs_dim, device


def _roll(rows=6, D=5, k=3, vn=None, obs=None, rewards=None):
    import torch
    sf, rf = vnz.slot_floats(rows, D), vnz.slot_floats(rows, 1)
    if obs is None:
        obs = torch.zeros((k + 1) * sf).as_strided((k + 1, rows, D), (sf, D, 1))
    if rewards is None:
        rewards = torch.zeros(k * rf).as_strided((k, rows), (rf, 1))
    return vnz.NormalizedRollout(vn or _Shape(rows, D), k, obs, rewards, True)


def test_slot_strides_are_multiples_of_16_bytes():
    assert vnz.slot_floats(6, 5) == 32 and vnz.slot_floats(3, 1) == 4 and vnz.slot_floats(8, 4) == 32


def test_normalised_rollout_validation_needs_no_gpu():
    import torch
    check = vnz.check_normalized_rollout
    with pytest.raises(TypeError, match='NormalizedRollout'):
        check(object(), 3, 6, 5, 0)
    # shape mismatch with the engine
    with pytest.raises(ValueError, match='holds 6 rows of 5 columns, the engine\'s rows are 7 of 5'):
        check(_roll(), 3, 7, 5, 0)
    with pytest.raises(ValueError, match='the engine\'s rows are 6 of 4'):
        check(_roll(), 3, 6, 4, 0)
    with pytest.raises(ValueError, match='lives on cuda:1'):
        check(_roll(vn=_Shape(6, 5, 1)), 3, 6, 5, 0)
    with pytest.raises(ValueError, match='dtype float32'):
        check(_roll(obs=torch.zeros((4, 6, 5), dtype=torch.float64)), 3, 6, 5, 0)
    with pytest.raises(ValueError, match='records have shape'):
        check(_roll(rewards=torch.zeros((3, 5))), 3, 6, 5, 0)
    with pytest.raises(ValueError, match='holds 4 records, the call needs 5'):
        check(_roll(), 4, 6, 5, 0)
    with pytest.raises(ValueError, match='holds 3 records, the call needs 4'):
        check(_roll(obs=torch.zeros(5 * 32).as_strided((5, 6, 5), (32, 5, 1))), 4, 6, 5, 0)
    with pytest.raises(ValueError, match='multiple of 16'):      # 30 floats: short of 16 bytes
        check(_roll(obs=torch.zeros((4, 6, 5))), 3, 6, 5, 0)
    with pytest.raises(ValueError, match='multiple of 16'):
        check(_roll(rewards=torch.zeros((3, 6))), 3, 6, 5, 0)
    with pytest.raises(ValueError, match='contiguous'):
        check(_roll(obs=torch.zeros((4, 6, 10))[:, :, ::2]), 3, 6, 5, 0)
    # everything about the form is right: the device check comes last
    with pytest.raises(ValueError, match='must be on device cuda:0'):
        check(_roll(), 3, 6, 5, 0)


def test_config_checks_in_python():
    for bad in (dict(rows=0), dict(obs_dim=0), dict(clip_obs=0), dict(clip_reward=-1),
                dict(gamma=float('nan')), dict(epsilon=-1.0)):
        kw = dict(rows=4, obs_dim=3, clip_obs=10., clip_reward=10., gamma=0.99, epsilon=1e-8)
        kw.update(bad)
        with pytest.raises(ValueError):
            vnz.check_config(**kw)


def test_noise_struct():
    from custom_envs_amd.rng import DeviceRng
    g = DeviceRng((7 << 32) | 5, None)
    g.t, g.row_offset = 9, 3
    ns = vnz.noise_struct(g, 40)
    assert (ns.kind, ns.seed, ns.t0, ns.row0) == (_native.CE_NOISE_GENERATED, (7 << 32) | 5, 9, 3)
    ns = vnz.noise_struct(None, 40)
    assert (ns.kind, ns.ptr, ns.stride) == (_native.CE_NOISE_BLOCK, None, 40)


# --------------------------------------------------------------- the wrapper
class _StubMultiEnv:
    def __init__(self, agents=2):
        from custom_envs_amd.spaces import Box, Dict
        names = ['parameter-%d' % i for i in range(agents)]
        self.observation_space = Dict({n: Box(-1e3, 1e3, (4,)) for n in names})
        self.action_space = Dict({n: Box(-1e3, 1e3, (1,)) for n in names})

    def reset(self):
        return {n: np.zeros(4, np.float32) for n in self.observation_space.spaces}

    def close(self):
        pass


def test_wrapper_rejects_what_it_cannot_wrap():
    from custom_envs_amd.vectorize import OptVecEnv, VecNormalize
    venv = OptVecEnv([functools.partial(_StubMultiEnv, 2)])
    assert not venv.engine_backed
    with pytest.raises(TypeError, match='engine-backed OptVecEnv'):
        VecNormalize(venv)
    venv.close()
    with pytest.raises(TypeError, match='got list'):
        VecNormalize([])


def test_env_spec_refuses_a_stranger_and_names_the_wrapper():
    from custom_envs_amd.agents import env_spec
    with pytest.raises(TypeError, match='GPUVecEnv or an engine-backed OptVecEnv'):
        env_spec(object())
    assert 'VecNormalize' in env_spec.__doc__


def _bare_wrapper():
    from custom_envs_amd.vectorize import VecNormalize
    return object.__new__(VecNormalize)        # no device: only the refusals are called


def test_collect_ddpg_and_ddpg_raise():
    from custom_envs_amd import ddpg
    from custom_envs_amd.agents import DDPG
    wrapped = _bare_wrapper()
    with pytest.raises(NotImplementedError, match='collect_ddpg'):
        wrapped.collect_ddpg(None, None, 4)
    with pytest.raises(ValueError, match='DDPG on a VecNormalize env'):
        DDPG(ddpg.MlpPolicy, wrapped)


def test_distribute_raises():
    from custom_envs_amd.agents import A2C, PPO2, EnvSpec, MlpPolicy
    for cls in (PPO2, A2C):
        model = cls(MlpPolicy, EnvSpec(4, 5, 2, device=None), seed=1)
        model.env = _bare_wrapper()
        with pytest.raises(NotImplementedError, match='VecNormalize'):
            model.distribute(0, 1, broadcast=False)
        assert model.dist is None


def test_sb_pickles_are_refused(tmp_path):
    wrapped = _bare_wrapper()
    (tmp_path / 'obs_rms.pkl').write_bytes(b'')
    with pytest.raises(NotImplementedError, match='pickled'):
        wrapped.load_running_average(tmp_path)
    with pytest.raises(FileNotFoundError):
        wrapped.load_running_average(tmp_path / 'nowhere')
