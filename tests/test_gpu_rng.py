"""The counter-based generator on the device (csrc/rng.h) against its NumPy
statement (custom_envs_amd/rng.py), and the policy kernel's generated-noise
instance against the explicit-noise one, bit for bit.

Shapes where the kernel can go wrong: rows 1, 33 (a tile edge) and 70 (a
ragged third tile); act_dim 1, 3 (a partial block), 4 (one block), 20 and 64
(the 8-thread neglogp sums wrap); hidden (32,), (64, 64), (96,) (the fourth
wave idle) and (32, 128) (growing); t0 and row0 non-zero; a seed with a
non-zero high word.

The normals' bound, 1e-5 absolute against the float64 statement: every
argument of logf / log1pf / sincospif is exact (rng.h), the functions are
within 2 ulp, and |z| <= 5.89, which gives about 4e-6.
"""
import numpy as np
import pytest

import policy_cases as pc
from custom_envs_amd import rng
from custom_envs_amd.policy import POLICY_FIELDS, MlpPolicy

pytestmark = pytest.mark.gpu

SEED = (0x9e3779b9 << 32) | 0x1234567          # a non-zero high word
ROWS = (1, 33, 70)
ACT_DIMS = (1, 3, 4, 20, 64)


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


# ------------------------------------------------ 1. generator == its statement
@pytest.mark.parametrize('n', [1, 3, 4, 1000, 70001])
def test_u32_equals_statement(n):
    g = rng.DeviceRng(SEED, 0)
    for purpose, t in ((rng.PERMUTATION, 0), (rng.PREDICT, 2 ** 32 - 1), (7, 12345)):
        got = _np(g.u32(purpose, t, n))
        assert np.array_equal(got.astype(np.uint32), rng.u32_numpy(SEED, purpose, t, n))


def test_permutation_equals_statement():
    g = rng.DeviceRng(SEED, 0)
    for epoch in range(3):
        assert g.epoch == epoch
        got = _np(g.permutation(97))
        assert got.dtype == np.int32
        assert np.array_equal(got, rng.permutation_numpy(SEED, epoch, 97))
    assert g.t == 0


@pytest.mark.parametrize('act_dim', ACT_DIMS)
@pytest.mark.parametrize('rows', ROWS)
def test_normal_against_statement(rows, act_dim):
    g = rng.DeviceRng(SEED, 0, row_offset=1000003)
    g.t = 2 ** 31 + 5
    k = 3
    got = _np(g.normal(k, rows, act_dim)).astype(np.float64)
    assert g.t == 2 ** 31 + 5                    # normal() does not advance
    ref = np.stack([rng.normal_numpy(SEED, g.t + s, rows, act_dim, row_offset=1000003)
                    for s in range(k)])
    worst = float(np.abs(got - ref).max())
    print('normal vs statement rows %d A %d: worst %.3e' % (rows, act_dim, worst))
    assert worst <= 1e-5
    assert np.abs(got).max() <= 5.89


def test_normal_extreme_words_and_moments():
    """A block large enough to hold words near both ends of u (where a
    rounded float32 u would fail the bound), and its moments."""
    g = rng.DeviceRng(SEED, 0)
    rows, A, k = 4096, 64, 4
    got = _np(g.normal(k, rows, A)).astype(np.float64)
    ref = np.stack([rng.normal_numpy(SEED, s, rows, A) for s in range(k)])
    worst = float(np.abs(got - ref).max())
    print('normal vs statement, %d values: worst %.3e' % (got.size, worst))
    assert worst <= 1e-5
    assert abs(got.mean()) < 4e-3 and abs(got.std() - 1.0) < 4e-3      # 4 sigma of 2^20 values


def test_normal_strided_records():
    import torch
    from custom_envs_amd import _native
    rows, A, k = 33, 3, 2
    stride = 128                                 # floats per record; rows * A = 99
    buf = torch.full((k * stride,), 7.0, dtype=torch.float32, device='cuda')
    _native.check(_native.load().ce_rng_normal(buf.data_ptr(), k, rows, A, stride * 4, SEED, 5, 9,
                                               torch.cuda.current_stream().cuda_stream), 'normal')
    torch.cuda.synchronize()
    got = _np(buf).reshape(k, stride)
    g = rng.DeviceRng(SEED, 0, row_offset=9)
    g.t = 5
    assert np.array_equal(got[:, :rows * A].reshape(k, rows, A), _np(g.normal(k, rows, A)))
    assert np.all(got[:, rows * A:] == 7.0)      # nothing past a record is written


# ---------------------------- 2. forward_device(noise=rng) == explicit, bit for bit
@pytest.mark.parametrize('hidden', [(32,), (64, 64), (96,), (32, 128)],
                         ids=['h32', 'h64x64', 'h96', 'h32x128'])
@pytest.mark.parametrize('act_dim', ACT_DIMS)
@pytest.mark.parametrize('rows', ROWS)
def test_forward_generated_equals_explicit(rows, act_dim, hidden):
    import torch
    D = 13
    rs = np.random.RandomState(rows * 100 + act_dim)
    policy = MlpPolicy(D, act_dim, hidden, low=-0.5, high=0.5)
    policy.set_params(pc.draw_params(rs, D, act_dim, hidden))
    obs = torch.from_numpy(rs.normal(0, 1, (rows, D)).astype(np.float32)).cuda()
    g = rng.DeviceRng(SEED, 0, row_offset=77)
    g.t = 41
    explicit = policy.forward_device(obs, noise=g.normal(1, rows, act_dim)[0])
    generated = policy.forward_device(obs, noise=g)
    torch.cuda.synchronize()
    assert g.t == 41
    for name in POLICY_FIELDS:
        assert np.array_equal(_bits(_np(generated[name])), _bits(_np(explicit[name]))), name
    assert np.isfinite(_np(generated['neglogp'])).all()
    # the noise was used: the sample differs from the mean
    mean = policy.forward_device(obs)
    assert not np.array_equal(_np(mean['action']), _np(generated['action']))
    policy.close()


def test_forward_refuses_a_generator_elsewhere_or_spent():
    import torch
    policy = MlpPolicy(5, 2, (32,))
    obs = torch.zeros((3, 5), dtype=torch.float32, device='cuda')
    with pytest.raises(ValueError, match='generator lives on'):
        policy.forward_device(obs, noise=rng.DeviceRng(1, None))
    g = rng.DeviceRng(1, 0)
    g.t = 2 ** 32
    with pytest.raises(ValueError, match='2\\^32'):
        policy.forward_device(obs, noise=g)
    policy.close()


# ------------------------------------ 3. rollout_policy with a DeviceRng == tensor
def _make_engine(name):
    kind, kw = pc.ROLLOUT_SHAPES[name]
    if kind == 'optimize':
        from custom_envs_amd.engine import OptimizeEngine
        features, targets = pc.rollout_dataset(name)
        eng = OptimizeEngine(features, targets, num_envs=len(kw['seeds']),
                             batch_size=kw['batch_size'], max_steps=4)
        eng.seed(list(kw['seeds']))
        return eng
    from custom_envs_amd.multi_engine import MultiOptEngine
    return MultiOptEngine(kw['num_envs'], kw['problem'], max_batches=4, max_history=5)


def _rollout(name, generated, k=6):
    import torch
    eng = _make_engine(name)
    rows, D, A = pc.rollout_dims(name)
    params, _ = pc.rollout_policy_inputs(name)
    policy = MlpPolicy(D, A, pc.ROLLOUT_HIDDEN)
    policy.set_params(params)
    g = rng.DeviceRng(SEED, 0, row_offset=5)
    g.t = 9
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng.set_stream(stream.cuda_stream)
        first = eng.alloc_device_outputs()
        eng.reset_device(first)
        fields, rec, pfields, prec = eng.alloc_policy_rollout(k, policy)
        noise = g if generated else g.normal(k, rows, A, stream=stream.cuda_stream)
        eng.rollout_policy(k, policy, first['obs'], noise, fields, rec, pfields, prec)
        stream.synchronize()
        out = ({n: _np(fields[n]) for n, _, _, _ in eng.output_fields()},
               {n: _np(pfields[n]) for n in POLICY_FIELDS})
    assert g.t == 9                              # the caller advances
    eng.close()
    policy.close()
    return out


@pytest.mark.parametrize('name', ['lr_two_class_f64', 'multi_func4'])
def test_rollout_generated_equals_explicit(name):
    env_g, pol_g = _rollout(name, True)
    env_e, pol_e = _rollout(name, False)
    for n in pol_e:
        assert np.array_equal(_bits(pol_g[n]), _bits(pol_e[n])), n
    for n in env_e:
        assert np.array_equal(_bits(env_g[n]), _bits(env_e[n])), n
    assert env_g['done'].sum() >= env_g['done'].shape[1]         # across an auto-reset
    assert np.isfinite(pol_g['action']).all()


def test_rollout_refuses_a_spent_generator():
    import torch
    name = 'multi_func4'
    eng = _make_engine(name)
    rows, D, A = pc.rollout_dims(name)
    policy = MlpPolicy(D, A, pc.ROLLOUT_HIDDEN)
    first = eng.alloc_device_outputs()
    eng.reset_device(first)
    fields, rec, pfields, prec = eng.alloc_policy_rollout(2, policy)
    torch.cuda.synchronize()
    g = rng.DeviceRng(1, 0)
    g.t = 2 ** 32 - 1
    with pytest.raises(ValueError, match='2\\^32'):
        eng.rollout_policy(2, policy, first['obs'], g, fields, rec, pfields, prec)
    eng.close()
    policy.close()
