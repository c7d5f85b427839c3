"""What the act side costs at the reference's default Optimize-v0 shape
(49 features x 10 classes: a 981-wide observation, 490 actions), next to the
env step it drives.  WideMlpPolicy, hidden (64, 64).

  (a) WideMlpPolicy.forward_device at 4096 rows: the explicit instance (a
      noise tensor) and the generated one (a DeviceRng)
  (b) the same network in eager torch (policy_rollout_bench.EagerPolicy:
      Linear / tanh, torch.randn, clamp, the neg-log-prob)
  (c) on a full-batch float64 49 x 10 engine (a synthetic classification set,
      --rows rows, --envs envs): GPUVecEnv.collect(K) per step against
      step_device alone with fixed actions

Method: every leg is warmed up, then the legs run alternately, --repeats
repeats each, every repeat at least --min-seconds long and ended by a device
synchronise; min / median / max over the repeats.

    python scripts/wide_policy_bench.py --out profiles/r22_wide_policy.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if path not in sys.path:
        sys.path.insert(0, path)

from policy_rollout_bench import EagerPolicy, draw_params, time_calls  # noqa: E402

HIDDEN = (64, 64)
FEATURES, CLASSES = 49, 10
D, A = 2 * FEATURES * CLASSES + 1, FEATURES * CLASSES


def classification(n_rows, seed=0):
    rs = np.random.RandomState(seed)
    x = rs.normal(0, 1, (n_rows, FEATURES))
    y = np.argmax(x @ rs.normal(0, 1, (FEATURES, CLASSES)) + rs.normal(0, 0.5, (n_rows, CLASSES)),
                  axis=1)
    y[:CLASSES] = np.arange(CLASSES)
    return x, np.eye(CLASSES)[y]


def measure(legs, units, repeats, min_seconds, stream):
    """legs: name -> callable; units: name -> steps (or forwards) per call.
    Returns name -> {'us': {min, median, max}, ...} per unit."""
    calls = {}
    for name, fn in legs.items():
        time_calls(fn, 3, stream)
        n = 2
        while True:
            dt = time_calls(fn, n, stream)
            if dt >= 0.25 * min_seconds:
                break
            n *= 2
        calls[name] = max(1, int(np.ceil(n * min_seconds * 1.3 / dt)))
    samples = {name: [] for name in legs}
    for _ in range(repeats):
        for name, fn in legs.items():
            dt = time_calls(fn, calls[name], stream)
            while dt < min_seconds:
                calls[name] = int(np.ceil(calls[name] * 1.3 * min_seconds / dt))
                dt = time_calls(fn, calls[name], stream)
            samples[name].append(dt / (calls[name] * units[name]))
    out = {}
    for name, vals in samples.items():
        us = np.array(vals) * 1e6
        out[name] = {'us': {'min': float(us.min()), 'median': float(np.median(us)),
                            'max': float(us.max())},
                     'calls_per_repeat': calls[name], 'repeats': repeats}
    return out


def forward_legs(rows, stream):
    import torch
    from custom_envs_amd.policy import WideMlpPolicy
    from custom_envs_amd.rng import DeviceRng
    dev = torch.device('cuda', 0)
    policy = WideMlpPolicy(D, A, HIDDEN, low=-1e3, high=1e3)
    params = draw_params(policy.params_layout(), np.random.RandomState(7))
    policy.set_params(params)
    obs = torch.randn((rows, D), dtype=torch.float32, device=dev)
    noise = torch.randn((rows, A), dtype=torch.float32, device=dev)
    out = policy.alloc_outputs(rows)
    g = DeviceRng(11, 0)
    eager = EagerPolicy(params, len(HIDDEN), -1e3, 1e3, dev)
    legs = {'a_forward_explicit': lambda: policy.forward_device(obs, noise, out=out),
            'a_forward_generated': lambda: policy.forward_device(obs, g, out=out),
            'b_eager_torch': lambda: eager(obs)}
    return legs, {name: 1 for name in legs}, (policy, out)


def collect_legs(envs, n_rows, k, stream):
    import torch
    from custom_envs_amd.policy import WideMlpPolicy
    from custom_envs_amd.vectorize.gpuvecenv import GPUVecEnv
    dev = torch.device('cuda', 0)
    env = GPUVecEnv(envs, data_set=classification(n_rows), max_steps=40, seed=0, precision='f64')
    eng = env.engine
    assert (eng.obs_dim, eng.act_dim) == (D, A)
    policy = WideMlpPolicy(D, A, HIDDEN, low=-1e3, high=1e3)
    policy.set_params(draw_params(policy.params_layout(), np.random.RandomState(7)))
    env.reset()
    noise = torch.randn((k, envs, A), dtype=torch.float32, device=dev)
    fixed = (0.01 * torch.randn((k, envs, A), dtype=torch.float32, device=dev)).contiguous()
    out = eng.alloc_device_outputs()

    def leg_collect():
        env.collect(policy, k, noise)

    def leg_step():
        for t in range(k):
            eng.step_device(fixed[t], out)
        eng.wait()

    legs = {'c_collect': leg_collect, 'c_step_device_alone': leg_step}
    return legs, {name: k for name in legs}, (env, policy, out)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--min-seconds', type=float, default=0.5)
    ap.add_argument('--forward-rows', type=int, default=4096)
    ap.add_argument('--envs', type=int, default=256)
    ap.add_argument('--rows', type=int, default=1024)
    ap.add_argument('--k', type=int, default=16)
    args = ap.parse_args()
    doc = {'policy': {'obs_dim': D, 'act_dim': A, 'hidden': list(HIDDEN)}}
    stream = torch.cuda.current_stream()
    legs, units, keep = forward_legs(args.forward_rows, stream)
    doc['forward'] = {'rows': args.forward_rows, 'unit': 'us per forward',
                      'legs': measure(legs, units, args.repeats, args.min_seconds, stream)}
    legs, units, keep = collect_legs(args.envs, args.rows, args.k, stream)
    doc['collect'] = {'envs': args.envs, 'dataset_rows': args.rows, 'k': args.k,
                      'unit': 'us per env step (all envs)',
                      'legs': measure(legs, units, args.repeats, args.min_seconds, stream)}
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(doc))


if __name__ == '__main__':
    main()
