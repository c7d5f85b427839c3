"""The K-step kernel's register-held gradient operands (CE_LP_GA_REGS,
csrc/optimize_lr_persist.h): a row wave forms each tile's gradient A
operands in one LDS transposition tile, reads them back once in the prologue
and keeps them in VGPRs for the whole launch (the 16x16x4 form keeps its own
lanes' values without the round trip).

Every test compares a K-step launch byte for byte with K one-step launches
(set_persistent(False)): every field of every step's record and get_state.
Each shape first asserts that the K-step engine runs
optimize_lr_persist_ws_kernel (many_kernel) in the instance named beside it;
the one-step kernel is held to its 4-wave form, the K-step kernel's
tile -> wave split.

The datasets are random normal, so every tile differs and a tile taken for
another changes the gradient.  max_steps = 5, E = 40 (two full workgroups and
one of 8 envs), K = 3 and K = 7 (the second crosses an auto-reset).  The
shapes are the smallest for each way the operand fill can go:

  256 x 10   <3,4,false>  the benchmark instance: four tiles per wave
  64 x 7     <2,1,false>  one tile per wave, masked feature lanes
  128 x 5    <2,2,false>  two tiles per wave
  100 x 10   <3,2,true>   7 tiles: row wave 3 holds a dead second tile (zeros)
  208 x 9    <3,4,true>   13 tiles: three row waves hold a dead fourth tile;
                          the instance with the most registers
  36 x 3     <1,1,true>   3 tiles: row wave 3 has no tile at all
  128 x 13   <4,2,false>  four feature groups: the 16x16x4 form

One more shape, 64 x 16 at E = 21 (<4,1,false>), takes the two paths of the
epilogue waves' observation flush that E = 40 at these widths does not
reach: the full workgroup's block is 260 16-byte units for 256 threads (a
second pass of the store loop), the 5-env workgroup's 325 floats end in a
one-float tail.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ('obs', 'reward', 'done', 'objective', 'accuracy', 'episode_len')
STATE = ('weights', 'grad_hist', 'loss_hist', 'step', 'init_weights')
WS = 'optimize_lr_persist_ws_kernel<'
E, T = 40, 7

SHAPES = [
    (256, 10, '3,4,false>'),
    (64, 7, '2,1,false>'),
    (128, 5, '2,2,false>'),
    (100, 10, '3,2,true>'),
    (208, 9, '3,4,true>'),
    (36, 3, '1,1,true>'),
    (128, 13, '4,2,false>'),
]


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')


@pytest.fixture(autouse=True)
def _four_wave_one_step(monkeypatch):
    # at these env counts the one-step kernel would pick 8 waves, whose
    # partials meet in another order than the K-step kernel's 4 row waves
    monkeypatch.setenv('CE_LR_WAVES', '4')


def _dataset(n_rows, n_features):
    rs = np.random.RandomState(7 * n_rows + n_features)
    x = rs.normal(0, 1, (n_rows, n_features))
    y = (x @ rs.normal(0, 1, n_features) + rs.normal(0, 0.5, n_rows) > 0).astype(np.int64)
    return x, np.eye(2)[y]


def _acts(n_rows, n_features, E=E):
    rs = np.random.RandomState(n_rows + 31 * n_features)
    return rs.normal(0, 0.01, (T, E, 2 * n_features)).astype(np.float32)


def _engine(data, persistent, E=E):
    from custom_envs_amd.engine import OptimizeEngine
    eng = OptimizeEngine(*data, num_envs=E, max_steps=5)
    eng.set_persistent(persistent)
    if persistent:
        assert eng.many_kernel.startswith(WS), eng.many_kernel
    else:
        assert eng.step_kernel.endswith(',4>'), eng.step_kernel
        assert not eng.persistent
    eng.seed(list(range(E)))
    eng.reset()
    return eng


def _launch(eng, k, dact):
    """One K-step call from the engine's current state: every step's record
    as numpy [k][E...]."""
    fields, rb = eng.alloc_rollout(k)
    eng.rollout_device(k, dact, fields, rb)
    eng.wait()
    return {name: fields[name].cpu().numpy() for name in FIELDS}


_ref_cache = {}


def _reference(n_rows, n_features, E=E):
    """The T one-step launches of one shape, once (shared, read only):
    (records [T][E...], the state after every step)."""
    import torch
    key = (n_rows, n_features, E)
    if key not in _ref_cache:
        eng = _engine(_dataset(n_rows, n_features), False, E)
        dact = torch.from_numpy(_acts(n_rows, n_features, E)).cuda()
        recs, states = [], []
        for t in range(T):
            recs.append(_launch(eng, 1, dact[t:t + 1]))
            states.append(eng.get_state())
        eng.close()
        _ref_cache[key] = ({n: np.concatenate([r[n] for r in recs]) for n in FIELDS}, states)
    return _ref_cache[key]


def _same(got, ref, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    assert got.tobytes() == ref.tobytes(), what


def _compare(n_rows, n_features, kernel, K, E=E):
    import torch
    ref, ref_states = _reference(n_rows, n_features, E)
    eng = _engine(_dataset(n_rows, n_features), True, E)
    assert eng.many_kernel == WS + kernel
    got = _launch(eng, K, torch.from_numpy(_acts(n_rows, n_features, E)[:K].copy()).cuda())
    st = eng.get_state()
    eng.close()
    what = '%dx%d E=%d K=%d' % (n_rows, n_features, E, K)
    for name in FIELDS:
        _same(got[name], ref[name][:K], '%s %s' % (what, name))
    for name in STATE:
        _same(st[name], ref_states[K - 1][name], '%s state %s' % (what, name))
    return got


@pytest.mark.parametrize('K', [3, 7])
def test_wide_observation_block_and_float_tail(K):
    _compare(64, 16, '4,1,false>', K, E=21)


@pytest.mark.parametrize('K', [3, 7])
@pytest.mark.parametrize('n_rows,n_features,kernel', SHAPES)
def test_k_steps_equal_one_step_launches(n_rows, n_features, kernel, K):
    got = _compare(n_rows, n_features, kernel, K)
    if K == 7:
        # the launch crossed the auto-reset at step 5
        assert got['episode_len'][:, E - 1].tolist() == [1, 2, 3, 4, 5, 1, 2]
        assert got['done'][:, E - 1].tolist() == [0, 0, 0, 0, 1, 0, 0]
