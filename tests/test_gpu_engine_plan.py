"""One tiny engine per kernel path (csrc/engine_plan.h: Register, Gen, LrMfma,
MlpFused, Net), 4 envs each: the engine reports the kernels ce_test_plan
plans for the same config and switches, its state round-trips through
set_state / get_state, and a reset plus two steps match the oracle at the
tolerances of the path's own suite (test_gpu_paths.py for the linear
problem, test_gpu_mlp.py for the networks).
"""
import numpy as np
import pytest

from custom_envs_amd.engine import make_config

pytestmark = pytest.mark.gpu

E = 4


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')


def _linear(n_rows, n_features, n_classes, seed):
    rs = np.random.RandomState(seed)
    y = np.arange(n_rows) % n_classes
    x = rs.normal(0, 1, (n_classes, n_features))[y] + rs.normal(0, 1, (n_rows, n_features))
    return x, np.eye(n_classes)[y]


def _mlp():
    from oracle.gen_golden import mlp_dataset
    return mlp_dataset()          # 128 x 16, 10 classes


# path: (dataset, engine arguments, switches)
CASES = {
    'register': (lambda: _linear(8, 3, 3, 1), dict(batch_size=4), {}),
    'gen': (lambda: _linear(8, 3, 3, 1), dict(batch_size=4), {'CE_GENERIC': '1'}),
    'lr': (lambda: _linear(16, 10, 2, 2), dict(batch_size=None), {}),
    'fused': (_mlp, dict(batch_size=32, model='mlp', hidden=64), {}),
    'net': (_mlp, dict(batch_size=32, model='mlp', hidden=64), {'CE_MLP_NET': '1'}),
}
FAMILY = {'register': 'optimize_step_kernel<double,3,3,', 'gen': 'optimize_mfma_kernel<1>',
          'lr': 'optimize_lr_mfma_kernel<3,', 'fused': 'mlp_step_kernel', 'net': 'net<16,64,10>:mfma'}


@pytest.mark.parametrize('path', sorted(CASES))
def test_path(path, monkeypatch):
    from custom_envs_amd.engine import OptimizeEngine
    from test_engine_plan import CE_SWITCHES, _plan
    make_data, kwargs, env = CASES[path]
    features, targets = make_data()
    for name in CE_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = OptimizeEngine(features, targets, num_envs=E, **kwargs)
    try:
        cfg = make_config(len(features), features.shape[1], targets.shape[1], E, **kwargs)
        rc, step, many = _plan(cfg, np.argmax(targets, axis=1))
        assert rc == 0
        assert (eng.step_kernel, eng.many_kernel) == (step, many)
        assert step.startswith(FAMILY[path])
        assert eng.persistent == (path == 'lr')
        _two_steps_match_oracle(eng, features, targets, kwargs)
        _state_round_trip(eng, float32=kwargs.get('model') == 'mlp')
    finally:
        eng.close()


def _two_steps_match_oracle(eng, features, targets, kwargs):
    seeds = [31, 32, 33, 34]
    if kwargs.get('model') == 'mlp':
        from test_gpu_mlp import _net_check
        _net_check(features, targets, eng, (kwargs['hidden'],), kwargs['batch_size'], seeds, 2)
        return
    from test_gpu_paths import _check_against_oracle
    acts = np.random.RandomState(5).normal(0, 0.05, (2, E, eng.act_dim)).astype(np.float32)
    eng.seed(seeds)
    assert np.all(eng.reset() == 0)
    outs = [{k: v.copy() for k, v in eng.step(acts[t]).items()} for t in range(2)]
    _check_against_oracle((features, targets), kwargs['batch_size'], seeds, acts, outs, range(E))


def _state_round_trip(eng, float32):
    """Random weights, init weights and grad history come back exactly: as
    given where the path stores float64, rounded to float32 where it stores
    float32 (the MLP problem's W / W0; its grad history is float64), with
    nothing of the network path's zero-padded weight images leaking."""
    rs = np.random.RandomState(9)
    shape = (E, eng.act_dim)
    state = {k: rs.normal(0, 1, shape) for k in ('weights', 'init_weights', 'grad_hist')}
    eng.set_state(**state)
    got = eng.get_state()
    for name, sent in state.items():
        stored32 = float32 and name != 'grad_hist'
        want = sent.astype(np.float32).astype(np.float64) if stored32 else sent
        assert got[name].shape == shape and np.array_equal(got[name], want), name
