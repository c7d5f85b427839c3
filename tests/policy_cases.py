"""Inputs shared by the policy tests (test_policy_host.py, test_gpu_policy.py):
the parameter draws of the forward-parity cases and the closed-loop rollout
shapes with their policies.  Not a test module."""
import numpy as np

from custom_envs_amd.policy import params_layout

# (rows, D, hidden, A): one row; a tile and one row; two tiles and a tail with
# a 20-wide head; five tiles with a 1-wide head; the widest supported network
FORWARD_CASES = [(1, 5, (32,), 2), (33, 5, (32,), 2), (70, 41, (64, 64), 20),
                 (130, 15, (64, 64), 1), (257, 128, (128, 128, 128), 64)]

# The shapes FORWARD_CASES leaves out (its hidden widths are equal and powers
# of two): one 96 layer (the fourth wave idle); growing widths, the head one
# column into the second wave, D no multiple of 32; D wider than every layer
# over three unequal layers; shrink then grow with a head of exactly 32; 96 ->
# 96 (9 and 12 dW blocks over 4 waves, D = 100 a partial last row block);
# D = 4 with every width once and a 1-wide head
FORWARD_SHAPE_CASES = [(65, 7, (96,), 3), (65, 41, (32, 128), 33), (70, 128, (32, 64, 96), 5),
                       (40, 12, (128, 32, 64), 32), (70, 100, (96, 96), 64),
                       (33, 4, (64, 96, 128), 1)]


FORWARD_IDS = ['r%d_d%d_a%d' % (c[0], c[1], c[3]) for c in FORWARD_CASES]
FORWARD_SHAPE_IDS = ['r%d_d%d_h%s_a%d' % (c[0], c[1], 'x'.join(map(str, c[2])), c[3])
                     for c in FORWARD_SHAPE_CASES]


def draw_params(rs, obs_dim, act_dim, hidden, final_scale=1.0, logstd=None):
    """Weights N(0,1)/sqrt(fan_in), biases 0.1 N(0,1), logstd ~ U(-1, 0) (or
    the constant given); the two heads' weights times ``final_scale``.
    float32, as the dict of ``params_layout``."""
    params = {}
    for name, (_, shape) in params_layout(obs_dim, act_dim, hidden).items():
        if name == 'logstd':
            value = rs.uniform(-1, 0, shape) if logstd is None else np.full(shape, logstd)
        elif len(shape) == 2:
            value = rs.normal(0, 1, shape) / np.sqrt(shape[0])
            if name.endswith('w_out'):
                value = value * final_scale
        else:
            value = 0.1 * rs.normal(0, 1, shape)
        params[name] = value.astype(np.float32)
    return params


def forward_inputs(case, seed=0):
    """(obs, noise, params) of one forward-parity case, all float32: obs
    2 N(0,1) with every 7th row times 50 (saturated tanh), noise N(0,1)."""
    rows, D, hidden, A = case
    rs = np.random.RandomState(1000 + seed)
    params = draw_params(rs, D, A, hidden)
    obs = 2.0 * rs.normal(0, 1, (rows, D))
    obs[::7] *= 50.0
    noise = rs.normal(0, 1, (rows, A))
    return obs.astype(np.float32), noise.astype(np.float32), params


def rel_err(got, ref):
    """max|d| / max|ref| over a whole array (the project's float32 bound)."""
    ref = np.asarray(ref, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - ref)) / np.max(np.abs(ref)))


# ------------------------------------------------------------ rollout shapes
ROLLOUT_K = 10
ROLLOUT_HIDDEN = (64, 64)
ROLLOUT_LOGSTD = float(np.log(0.05))


def _classification(n_rows, n_features, n_classes, seed):
    rs = np.random.RandomState(seed)
    x = rs.normal(0, 1, (n_rows, n_features))
    y = np.argmax(x @ rs.normal(0, 1, (n_features, n_classes)) + rs.normal(0, 0.5, (n_rows, n_classes)),
                  axis=1)
    y[:n_classes] = np.arange(n_classes)          # every class present
    return x, np.eye(n_classes)[y]


# name -> (kind, kwargs): 'optimize' (dataset, engine keywords, seeds) or
# 'multi' (problem, E); every episode is 4 steps, so K = 10 crosses two resets
ROLLOUT_SHAPES = {
    'lr_two_class_f64': ('optimize', dict(data=(32, 10, 2, 5), batch_size=None, seeds=[21, 22, 23])),
    'softmax_3_class_b8': ('optimize', dict(data=(32, 4, 3, 6), batch_size=8, seeds=[31, 32, 33])),
    'multi_func': ('multi', dict(problem='func', num_envs=3)),
    'multi_func4': ('multi', dict(problem='func4', num_envs=2)),
}


def rollout_dims(name):
    """(rows, obs_dim, act_dim) of a rollout shape."""
    kind, kw = ROLLOUT_SHAPES[name]
    if kind == 'optimize':
        _, F, K, _ = kw['data']
        return len(kw['seeds']), 2 * F * K + 1, F * K
    P = {'func': 2, 'func4': 4}[kw['problem']]
    return kw['num_envs'] * P, 15, 1


def rollout_dataset(name):
    return _classification(*ROLLOUT_SHAPES[name][1]['data'])


def rollout_policy_inputs(name):
    """(params dict, noise [K][rows][A]) of a rollout shape: head weights
    times 0.01 and logstd = log 0.05, so the envs stay finite."""
    rows, D, A = rollout_dims(name)
    rs = np.random.RandomState(sorted(ROLLOUT_SHAPES).index(name) + 50)
    params = draw_params(rs, D, A, ROLLOUT_HIDDEN, final_scale=0.01, logstd=ROLLOUT_LOGSTD)
    noise = rs.normal(0, 1, (ROLLOUT_K, rows, A)).astype(np.float32)
    return params, noise
