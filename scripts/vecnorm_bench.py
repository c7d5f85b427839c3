"""What the device VecNormalize adds to a rollout.

Workloads: config 2 (Optimize-v0, 256 x 10, two classes, float64) at 4096 envs
(4096 rows x 41 columns) and MultiOptLRs-v0 func4 at 1024 envs (4096 rows x 15
columns); the policy is stable-baselines' MlpPolicy shape, hidden (64, 64),
K = 128 steps per rollout, the noise generated in the policy kernel.

Legs, per workload:
  collect_plain    env.collect(policy, K, noise=DeviceRng): [policy, env] x K
  collect_vecnorm  VecNormalize(env).collect(...): [policy, env, normalise] x K
  vecnorm_alone    K ce_vecnorm_step launches back to back on one stream (the
                   kernel with its launch, nothing between the launches)

Method, as scripts/learn_bench.py: every leg is warmed up, then the legs run
alternately, five repeats each, every repeat at least --min-seconds long and
ended by a device synchronise; min / median / max over the repeats.  The plain
leg re-measures the parent's collect_rng figure (profiles/r15_learn.json) in
the same call.

    python scripts/vecnorm_bench.py --out profiles/r21_vecnorm.json
    python scripts/vecnorm_bench.py --trace        # a short run for a kernel trace

Whether normalisation improves learning on these envs is not measured here.
"""
import argparse
import functools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from learn_bench import HIDDEN, K, draw_params, time_calls  # noqa: E402


def make_env(workload, envs):
    if workload == 'config2':
        from custom_envs_amd.vectorize.gpuvecenv import GPUVecEnv
        return GPUVecEnv(envs, data_set='gaussians_256x10', seed=0)
    from custom_envs_amd.core import make
    from custom_envs_amd.vectorize.optvecenv import OptVecEnv
    env = OptVecEnv([functools.partial(make, 'MultiOptLRs-v0', problem='func4')] * envs)
    assert env.engine_backed
    return env


def build_legs(workload, envs):
    import torch
    from custom_envs_amd.agents import env_spec
    from custom_envs_amd.policy import MlpPolicy
    from custom_envs_amd.rng import DeviceRng
    from custom_envs_amd.vectorize.vecnormalize import DeviceVecNorm, VecNormalize

    plain = make_env(workload, envs)
    plain.reset()
    wrapped = VecNormalize(make_env(workload, envs))
    wrapped.reset()
    spec = env_spec(plain)
    policy = MlpPolicy(spec.obs_dim, spec.act_dim, HIDDEN, low=spec.low, high=spec.high)
    policy.set_params(draw_params(policy.params_layout(), np.random.RandomState(7)))
    gens = [DeviceRng(11, 0), DeviceRng(11, 0)]

    def wrap(gen):
        if gen.t + 2 * K > 2 ** 32:
            gen.t = 0

    def collect_plain():
        wrap(gens[0])
        plain.collect(policy, K, noise=gens[0])

    def collect_vecnorm():
        wrap(gens[1])
        wrapped.collect(policy, K, noise=gens[1])

    rows, D = spec.rows, spec.obs_dim
    vn = DeviceVecNorm(rows, D)
    obs = torch.randn((rows, D), dtype=torch.float32, device='cuda') * 100.0
    rew = -100.0 + 10.0 * torch.randn(rows, dtype=torch.float32, device='cuda')
    done = (torch.rand(rows, device='cuda') < 0.2).to(torch.uint8)
    obs_out, rew_out = torch.empty_like(obs), torch.empty_like(rew)
    stream = torch.cuda.current_stream().cuda_stream

    def vecnorm_alone():
        for _ in range(K):
            vn.step_device(obs, rew, done, obs_out=obs_out, reward_out=rew_out, stream=stream)

    legs = {'collect_plain': collect_plain, 'collect_vecnorm': collect_vecnorm,
            'vecnorm_alone': vecnorm_alone}
    return legs, (plain, wrapped, policy, vn), (rows, D)


def run_workload(workload, envs, repeats, min_seconds):
    legs, keep, (rows, D) = build_legs(workload, envs)
    calls = {}
    for name, fn in legs.items():               # warm up, then size a repeat
        time_calls(fn, 2)
        n = 2
        while True:
            dt = time_calls(fn, n)
            if dt >= 0.25 * min_seconds:
                break
            n *= 2
        calls[name] = max(1, int(np.ceil(n * min_seconds * 1.3 / dt)))
    samples = {name: [] for name in legs}
    for _ in range(repeats):                    # the legs alternately
        for name, fn in legs.items():
            dt = time_calls(fn, calls[name])
            while dt < min_seconds:
                calls[name] = int(np.ceil(calls[name] * 1.3 * min_seconds / dt))
                dt = time_calls(fn, calls[name])
            samples[name].append(dt / (calls[name] * K))
    out = {}
    for name, per_step in samples.items():
        us = np.array(per_step) * 1e6
        out[name] = {'us_per_step': {'min': float(us.min()), 'median': float(np.median(us)),
                                     'max': float(us.max())},
                     'calls_per_repeat': calls[name], 'repeats': repeats}
    added = out['collect_vecnorm']['us_per_step']['median'] - \
        out['collect_plain']['us_per_step']['median']
    state = keep[1].normalizer.get_state()
    assert np.isfinite(state['obs_mean']).all() and np.isfinite(state['obs_var']).all()
    keep[1].close(), keep[0].close()
    return {'envs': envs, 'rows': rows, 'obs_dim': D, 'legs': out,
            'added_us_per_step_median': float(added)}


def trace(envs_config2, envs_func4):
    """Two wrapped rollouts per workload and nothing else: what a kernel trace
    of the normaliser's own duration is taken from."""
    import torch
    for workload, envs in (('config2', envs_config2), ('func4', envs_func4)):
        legs, keep, _ = build_legs(workload, envs)
        for _ in range(2):
            legs['collect_vecnorm']()
        torch.cuda.synchronize()
        keep[1].close(), keep[0].close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--func4-envs', type=int, default=1024)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--min-seconds', type=float, default=1.0)
    ap.add_argument('--trace', action='store_true')
    args = ap.parse_args()
    if args.trace:
        trace(args.envs, args.func4_envs)
        return
    import torch
    doc = {'k': K, 'hidden': list(HIDDEN), 'device': torch.cuda.get_device_name(0),
           'note': 'us_per_step: a call\'s wall time / K (a call is K steps or K launches); '
                   'added_us_per_step_median: collect_vecnorm - collect_plain',
           'config2': run_workload('config2', args.envs, args.repeats, args.min_seconds),
           'func4': run_workload('func4', args.func4_envs, args.repeats, args.min_seconds)}
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(doc))


if __name__ == '__main__':
    main()
