"""The three row bodies of the two-class kernels (lr_tier, csrc/
optimize_lr_mfma.h): batched reciprocals while every lane's partial of the
|u| bound is below 40, clamp-free below 162.5, clamped otherwise.

Each case runs the same states and actions through ONE K-step launch and
through per-step launches (set_persistent(False), held to the 4-wave form,
the K-step kernel's tile -> wave split): every output of every step and the
final state equal bit for bit, and sampled envs equal the oracle at the
tolerances of tests/test_gpu_persist.py.  The tier a workgroup takes is not
observable from outside, so each case asserts, from the weights it sets and
the data's column maxima, the partial bounds that decide it.
"""
import numpy as np
import pytest

from oracle.optimize import Optimize as OracleEnv

pytestmark = pytest.mark.gpu

F64_RTOL = 1e-6
F64_ATOL = 1e-9
FIELDS = ('obs', 'reward', 'done', 'objective', 'accuracy', 'episode_len')
STATE = ('weights', 'grad_hist', 'loss_hist', 'step')


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')


def _dataset(n_rows, n_features, seed):
    rs = np.random.RandomState(seed)
    x = rs.normal(0, 1, (n_rows, n_features))
    y = (x @ rs.normal(0, 1, n_features) + rs.normal(0, 0.5, n_rows) > 0).astype(np.int64)
    return x, np.eye(2)[y]


def _partials(weights, action, xmax):
    """The kernels' per-lane partial bounds [E][4]: lane group h covers
    features 4k + h of W' = W - a."""
    F = xmax.size
    w = weights.reshape(len(weights), F, 2) - action.reshape(len(weights), F, 2).astype(np.float64)
    term = np.abs(w[:, :, 0] - w[:, :, 1]) * xmax
    return np.stack([term[:, h::4].sum(axis=1) for h in range(4)], axis=1)


def _run(data, E, K, acts, mutate, monkeypatch):
    """Per-step launches and one K-step launch from the same state: returns
    (outputs [K][E...], final state, the state the steps started from)."""
    import torch
    from custom_envs_amd.engine import OptimizeEngine
    monkeypatch.setenv('CE_LR_WAVES', '4')
    runs = []
    for persist in (False, True):
        eng = OptimizeEngine(*data, num_envs=E)
        eng.set_persistent(persist)
        if persist:
            assert eng.persistent, eng.many_kernel
        else:
            assert eng.step_kernel.endswith(',4>'), eng.step_kernel
        eng.seed(list(range(E)))
        eng.reset()
        st0 = eng.get_state()
        mutate(st0)
        eng.set_state(**{k: v for k, v in st0.items() if k != 'order'})
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            eng.set_stream(stream.cuda_stream)
            fields, rb = eng.alloc_rollout(K)
            eng.rollout_device(K, torch.from_numpy(acts).cuda(), fields, rb)
            stream.synchronize()
            got = {name: fields[name].cpu().numpy() for name in FIELDS}
        runs.append((got, eng.get_state()))
        eng.close()
    (a, sa), (b, sb) = runs
    for name in FIELDS:                      # bytes: a diverged env's NaNs compare too
        assert a[name].tobytes() == b[name].tobytes(), name
    for name in STATE:
        assert sa[name].tobytes() == sb[name].tobytes(), name
    return b, sb, st0


def _against_oracle(data, st0, acts, got, st, envs):
    F = data[0].shape[1]
    for i in envs:
        env = OracleEnv(*data)
        env.seed(i)
        env.reset()
        env.model.set_weights(st0['weights'][i].reshape(F, 2).copy())
        for t in range(len(acts)):
            obs, rew, done, info = env.step(acts[t, i])
            where = 'env %d step %d' % (i, t)
            assert np.all(np.isfinite(got['obs'][t, i])), where
            assert bool(got['done'][t, i]) == done, where
            assert got['episode_len'][t, i] == info['episode']['l'], where
            np.testing.assert_allclose(got['obs'][t, i], obs, rtol=F64_RTOL, atol=F64_ATOL, err_msg=where)
            assert got['reward'][t, i] == pytest.approx(rew, rel=F64_RTOL), where
            assert got['objective'][t, i] == pytest.approx(info['objective'], rel=F64_RTOL), where
            assert got['accuracy'][t, i] == np.float32(info['accuracy']), where
        np.testing.assert_allclose(st['weights'][i], env.model.weights.ravel(), rtol=1e-12, atol=1e-14)


def _acts(seed, K, E, P):
    return np.random.RandomState(seed).normal(0, 0.01, (K, E, P)).astype(np.float32)


def _margin_pair(magnitude):
    """(w_f0, w_f1) with w_f0 - w_f1 = magnitude (signed)."""
    return magnitude / 2, -magnitude / 2


@pytest.mark.parametrize('n_rows', [64, 256])
@pytest.mark.parametrize('E', [16, 17])
def test_batched_tier(E, n_rows, monkeypatch):
    """Fresh seeds, F = 10, K = 3: a full and a partial workgroup, one and
    four tiles per row wave, every workgroup on the batched body."""
    data = _dataset(n_rows, 10, 1000 + n_rows)
    xmax = np.abs(data[0]).max(axis=0)
    K, P = 3, 20
    acts = _acts(E + n_rows, K, E, P)
    got, st, st0 = _run(data, E, K, acts, lambda s: None, monkeypatch)
    assert _partials(st0['weights'], acts[0], xmax).max() < 39.0
    _against_oracle(data, st0, acts, got, st, range(E))


@pytest.mark.parametrize('partial', [100.0, 400.0])
def test_tier_boundaries(partial, monkeypatch):
    """32 envs, N = 256, K = 2: env 21 (second workgroup) carries a margin on
    feature 0 that puts lane group 0's partial between 40 and 162.5 (the
    clamp-free body) or above 162.5 (the clamped body); the first workgroup
    stays on the batched body.  Every env matches the oracle."""
    data = _dataset(256, 10, 77)
    xmax = np.abs(data[0]).max(axis=0)
    E, K, P, heavy = 32, 2, 20, 21
    acts = _acts(5, K, E, P)

    def mutate(s):
        s['weights'][heavy, 0:2] = _margin_pair(partial / xmax[0])

    got, st, st0 = _run(data, E, K, acts, mutate, monkeypatch)
    for t in range(K):                       # the actions move a partial by < 0.3
        pb = _partials(st0['weights'] - acts[:t].astype(np.float64).sum(axis=0), acts[t], xmax)
        assert pb[:16].max() < 39.0
        assert pb[16:].max() == pb[heavy, 0]
        assert (45.0 < pb[heavy, 0] < 160.0) if partial < 162.5 else pb[heavy, 0] > 170.0
    _against_oracle(data, st0, acts, got, st, range(E))


def test_top_of_batched_tier(monkeypatch):
    """One env whose four partials are each 38.5 (just under 40) against data
    whose rows 3, 7, 11, 15 and 77 hold the column maximum in every feature,
    signed so that the first four (one lane's four values of tile 0) reach
    u = -154 and row 77 u = +154: the batch's product of denominators is
    near 2^888 (the bound allows 2^924).  Every output is finite and equals
    the oracle's."""
    x, y = _dataset(256, 10, 78)
    sgn = np.random.RandomState(9).choice([-1.0, 1.0], 10)
    s_y = np.where(y[:, 0] == 1, 1.0, -1.0)  # u = s_y x . (w_0 - w_1)
    for r in (3, 7, 11, 15):
        x[r] = 4.5 * sgn * s_y[r]
    x[77] = -4.5 * sgn * s_y[77]
    data = (x, y)
    xmax = np.abs(x).max(axis=0)
    assert np.all(xmax == 4.5)
    E, K, P, heavy = 16, 2, 20, 6
    acts = _acts(6, K, E, P)

    def mutate(s):
        for f in range(10):
            share = 3 if f % 4 < 2 else 2    # features per lane group (F = 10)
            s['weights'][heavy, 2 * f:2 * f + 2] = _margin_pair(-sgn[f] * 38.5 / 4.5 / share)

    got, st, st0 = _run(data, E, K, acts, mutate, monkeypatch)
    pb = _partials(st0['weights'], acts[0], xmax)
    assert pb.max() < 39.5 and np.all(pb[heavy] > 38.0)
    w = st0['weights'][heavy].reshape(10, 2)
    u = s_y * (x @ (w[:, 0] - w[:, 1]))
    assert np.allclose(u[[3, 7, 11, 15]], -154.0, atol=0.5) and abs(u[77] - 154.0) < 0.5
    _against_oracle(data, st0, acts, got, st, range(E))


def test_padding_rows_inside_a_batch(monkeypatch):
    """N = 250: the last tile's rows 250..255 are padding, inside the batches
    of four of its lanes."""
    data = _dataset(250, 10, 79)
    xmax = np.abs(data[0]).max(axis=0)
    E, K, P = 16, 2, 20
    acts = _acts(7, K, E, P)
    got, st, st0 = _run(data, E, K, acts, lambda s: None, monkeypatch)
    assert _partials(st0['weights'], acts[0], xmax).max() < 39.0
    _against_oracle(data, st0, acts, got, st, range(E))


def test_diverged_weights_take_the_clamped_body(monkeypatch):
    """One env with an infinite weight: its workgroup runs the clamped body
    as before.  Its own outputs equal the per-step kernel's (bytes, in _run);
    the other envs of the workgroup match the oracle."""
    data = _dataset(256, 10, 80)
    E, K, P, bad = 16, 2, 20, 9
    acts = _acts(8, K, E, P)

    def mutate(s):
        s['weights'][bad, 4] = np.inf

    got, st, st0 = _run(data, E, K, acts, mutate, monkeypatch)
    assert not np.isfinite(_partials(st0['weights'], acts[0], np.abs(data[0]).max(axis=0))[bad]).all()
    _against_oracle(data, st0, acts, got, st, [i for i in range(E) if i != bad])
