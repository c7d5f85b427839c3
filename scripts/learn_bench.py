"""What the counter-based generator and the training loop cost.

Workload: config 2 (Optimize-v0, 256 x 10, two classes, float64) at 4096 envs,
the policy stable-baselines' MlpPolicy shape, hidden (64, 64), K = 128 steps
per rollout.

Legs:
  collect_randn     GPUVecEnv.collect(policy, K, noise=None): one torch.randn
                    [K][rows][A] per call, the explicit-noise policy kernel
  collect_rng       the same call with a DeviceRng: no noise tensor, the
                    generated-noise policy kernel
  forward_explicit  MlpPolicy.forward_device alone, noise a tensor
  forward_rng       MlpPolicy.forward_device alone, noise a DeviceRng
  randn_block       torch.randn [K][rows][A] alone (what collect_randn adds)
  rng_block         DeviceRng.normal(K, rows, A) alone (ce_rng_normal)
  learn_update      one whole PPO2.learn update (collect + update, n_steps = K)
  hand_update       the hand-written loop of the same update: collect with a
                    DeviceRng, PPO2Learner.update with DeviceRng permutations

Method, as scripts/policy_rollout_bench.py: every leg is warmed up, then the
legs run alternately, five repeats each, every repeat at least --min-seconds
long and ended by a device synchronise; min / median / max over the repeats.

    python scripts/learn_bench.py --out profiles/r15_learn.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

K = 128
HIDDEN = (64, 64)
ENVS = 4096


def draw_params(layout, rs):
    """N(0,1)/sqrt(fan_in) weights (heads x 0.01), 0.1 N(0,1) biases, logstd =
    log 0.05: small actions, so the envs stay finite over a long run."""
    params = {}
    for name, (_, shape) in layout.items():
        if name == 'logstd':
            value = np.full(shape, np.log(0.05))
        elif len(shape) == 2:
            value = rs.normal(0, 1, shape) / np.sqrt(shape[0]) * (0.01 if name.endswith('w_out') else 1.0)
        else:
            value = 0.1 * rs.normal(0, 1, shape)
        params[name] = value.astype(np.float32)
    return params


def build_legs(envs):
    import torch
    from custom_envs_amd.agents import PPO2, MlpPolicy as Marker
    from custom_envs_amd.policy import MlpPolicy, dict_to_flat
    from custom_envs_amd.ppo2 import PPO2Learner
    from custom_envs_amd.rng import DeviceRng
    from custom_envs_amd.vectorize.gpuvecenv import GPUVecEnv

    def make_env():
        env = GPUVecEnv(envs, data_set='gaussians_256x10', seed=0)
        env.reset()
        return env

    env = make_env()
    D, A = env.engine.obs_dim, env.engine.act_dim
    policy = MlpPolicy(D, A, HIDDEN, low=-1e3, high=1e3)
    params = draw_params(policy.params_layout(), np.random.RandomState(7))
    policy.set_params(params)
    flat = dict_to_flat(params, policy.params_layout())
    g = DeviceRng(11, 0)

    def wrap(gen):
        if gen.t + 2 * K > 2 ** 32:
            gen.t = 0

    def collect_randn():
        env.collect(policy, K, noise=None)

    def collect_rng():
        wrap(g)
        env.collect(policy, K, noise=g)

    obs = torch.randn((envs, D), dtype=torch.float32, device='cuda')
    noise = torch.randn((envs, A), dtype=torch.float32, device='cuda')
    pout = policy.alloc_outputs(envs)
    gf = DeviceRng(12, 0)

    def forward_explicit():
        for _ in range(K):
            policy.forward_device(obs, noise, out=pout)

    def forward_rng():
        for _ in range(K):
            policy.forward_device(obs, gf, out=pout)

    def randn_block():
        torch.randn((K, envs, A), dtype=torch.float32, device='cuda')

    def rng_block():
        gf.normal(K, envs, A)

    # the loop: a model and the hand-written form, each on its own env
    lenv = make_env()
    model = PPO2(Marker, lenv, n_steps=K, seed=5,
                 policy_kwargs={'net_arch': [dict(pi=list(HIDDEN), vf=list(HIDDEN))]})
    model.set_parameters(flat)
    n_batch = model.n_batch

    def learn_update():
        wrap(model.rng)
        model.learn(n_batch)

    henv = make_env()
    hpolicy = MlpPolicy(D, A, HIDDEN, low=-1e3, high=1e3)
    hlearner = PPO2Learner(hpolicy)
    hlearner.set_params(flat)
    hg = DeviceRng(5, 0)

    def hand_update():
        wrap(hg)
        result = henv.collect(hpolicy, K, noise=hg)
        perms = [hg.permutation(n_batch) for _ in range(4)]
        hlearner.update(result, noptepochs=4, nminibatches=4, perms=perms)

    legs = {'collect_randn': (collect_randn, K), 'collect_rng': (collect_rng, K),
            'forward_explicit': (forward_explicit, K), 'forward_rng': (forward_rng, K),
            'randn_block': (randn_block, K), 'rng_block': (rng_block, K),
            'learn_update': (learn_update, K), 'hand_update': (hand_update, K)}
    keep = (env, lenv, henv, policy, hpolicy, model, hlearner)
    return legs, keep


def time_calls(fn, calls):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def run(envs, repeats, min_seconds):
    import torch
    legs, keep = build_legs(envs)
    calls = {}
    for name, (fn, _) in legs.items():          # warm up, then size a repeat
        time_calls(fn, 2)
        n = 2
        while True:
            dt = time_calls(fn, n)
            if dt >= 0.25 * min_seconds:
                break
            n *= 2
        calls[name] = max(1, int(np.ceil(n * min_seconds * 1.3 / dt)))
    samples = {name: [] for name in legs}
    for _ in range(repeats):                     # the legs alternately
        for name, (fn, steps) in legs.items():
            dt = time_calls(fn, calls[name])
            while dt < min_seconds:
                calls[name] = int(np.ceil(calls[name] * 1.3 * min_seconds / dt))
                dt = time_calls(fn, calls[name])
            samples[name].append(dt / (calls[name] * steps))
    finite = bool(np.isfinite(keep[5].get_parameters()).all()
                  and np.isfinite(keep[6].get_params()).all())
    result = {}
    for name, per_step in samples.items():
        us = np.array(per_step) * 1e6
        result[name] = {'us_per_step': {'min': float(us.min()), 'median': float(np.median(us)),
                                        'max': float(us.max())},
                        'calls_per_repeat': calls[name], 'repeats': repeats}
    assert finite
    return {'envs': envs, 'k': K, 'hidden': list(HIDDEN),
            'device': torch.cuda.get_device_name(0),
            'note': 'us_per_step: a call\'s wall time / K (a call is K steps, K forwards or one '
                    '[K][rows][A] block)', 'legs': result}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--envs', type=int, default=ENVS)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--min-seconds', type=float, default=1.0)
    args = ap.parse_args()
    doc = run(args.envs, args.repeats, args.min_seconds)
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(doc))


if __name__ == '__main__':
    main()
