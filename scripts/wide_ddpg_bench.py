"""The wide DDPG agent (ddpg.WideDDPGAgent, csrc/ddpg_wide_kernels.h) at the
reference's default shape (Optimize-v0 on 49 features x 10 classes: a 981-wide
observation, 490 actions), hidden (64, 64).

Legs:
  act_explicit / act_generated   ``act`` over 4096 rows, the noise a tensor /
             formed in the kernel (Normal)
  A_train_N  one train step at batch N in eager torch on the same GPU
             (ddpg_update_bench.EagerDDPG: gather by index, the target
             networks, both losses, autograd, Adam on both blocks, the soft
             update)
  B_train_N  ``ReplayMemory.sample`` + ``WideDDPGAgent.step`` at batch N
for N = 128 (stable-baselines' batch) and N = 4096, over a memory of 8192
random records;
  sb_cycle   stable-baselines' cycle on a full-batch float64 49 x 10 engine
             (--envs envs, --rows rows of a synthetic classification set):
             ``collect_ddpg`` of 100 steps with generated Normal noise, then
             ``train`` of 50 steps at batch 128.

Method: every leg is warmed up, then the legs run alternately, `repeats`
repeats each, every repeat at least `min-seconds` long and ended by a device
synchronise; median (min - max) over the repeats.

    python scripts/wide_ddpg_bench.py --out profiles/r25_wide_ddpg.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'scripts')):
    if p not in sys.path:
        sys.path.insert(0, p)

from ddpg_update_bench import HIDDEN, HYPER, EagerDDPG, time_calls  # noqa: E402
from wide_policy_bench import A, D, classification  # noqa: E402

ACT_ROWS = 4096
MEMORY = 8192
BATCHES = (128, 4096)
ROLLOUT, TRAIN, SB_BATCH = 100, 50, 128
SCALE = 0.01


def build_legs(envs, rows):
    import torch
    from custom_envs_amd import ddpg
    from custom_envs_amd.rng import DeviceRng
    from custom_envs_amd.vectorize.gpuvecenv import GPUVecEnv
    dev = torch.device('cuda', 0)
    flat = ddpg.init_params_numpy(D, A, HIDDEN, seed=7)
    agent = ddpg.WideDDPGAgent(D, A, HIDDEN, scale=SCALE, **HYPER)
    agent.set_params(flat)
    eager = EagerDDPG(agent.params_layout(), flat, agent.n_actor, dev)
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1)
    memory = ddpg.ReplayMemory(MEMORY, MEMORY, D, A)
    memory.obs0.copy_(2 * torch.randn((MEMORY, D), device=dev, generator=gen))
    memory.obs1.copy_(2 * torch.randn((MEMORY, D), device=dev, generator=gen))
    memory.actions.copy_((0.5 * torch.randn((MEMORY, A), device=dev, generator=gen)).clamp_(-1, 1))
    memory.rewards.copy_(torch.randn(MEMORY, device=dev, generator=gen))
    memory.dones.copy_((torch.rand(MEMORY, device=dev, generator=gen) < 0.2).to(torch.uint8))
    memory.advance()
    obs = 2 * torch.randn((ACT_ROWS, D), device=dev, generator=gen)
    noise = 0.1 * torch.randn((ACT_ROWS, A), device=dev, generator=gen)
    out = {n: torch.empty((ACT_ROWS, A), device=dev) for n in ('action', 'env_action')}
    normal = ddpg.NormalActionNoise(np.zeros(A), 0.1 * np.ones(A))
    act_rng = DeviceRng(11, 0)
    legs = {'act_explicit': lambda: agent.act(obs, noise, out=out),
            'act_generated': lambda: agent.act(obs, noise=(normal, act_rng), out=out)}
    for n in BATCHES:
        legs['A_train_%d' % n] = lambda n=n: eager.train(memory, memory.sample(n, generator=gen))
        legs['B_train_%d' % n] = (
            lambda n=n: agent.step(memory.as_batch(), memory.sample(n, generator=gen)))

    # stable-baselines' cycle on an agent and a memory of its own
    env = GPUVecEnv(envs, data_set=classification(rows), max_steps=40, seed=0, precision='f64')
    assert (env.engine.obs_dim, env.engine.act_dim) == (D, A)
    cyc_agent = ddpg.WideDDPGAgent(D, A, HIDDEN, scale=SCALE, **HYPER)
    cyc_agent.set_params(flat)
    cyc_memory = ddpg.ReplayMemory(2 * ROLLOUT * envs, envs, D, A)
    cyc_rng = DeviceRng(12, 0)
    env.reset()

    def sb_cycle():
        env.collect_ddpg(cyc_agent, cyc_memory, ROLLOUT, noise=(normal, cyc_rng))
        cyc_agent.train(cyc_memory, TRAIN, SB_BATCH, cyc_rng)

    legs['sb_cycle'] = sb_cycle
    return legs, (agent, cyc_agent), eager, [env, memory, cyc_memory, obs, noise, out]


def run(repeats, min_seconds, envs, rows):
    import torch
    legs, agents, eager, keep = build_legs(envs, rows)
    calls = {}
    for name, fn in legs.items():             # warm up, then size a repeat to >= min_seconds
        time_calls(fn, 2)
        n = 1
        while True:
            dt = time_calls(fn, n)
            if dt >= 0.25 * min_seconds:
                break
            n *= 2
        calls[name] = max(1, int(np.ceil(n * min_seconds * 1.3 / dt)))
    samples = {name: [] for name in legs}
    for _ in range(repeats):                  # the legs alternately
        for name, fn in legs.items():
            dt = time_calls(fn, calls[name])
            while dt < min_seconds:            # a short repeat is discarded and redone longer
                calls[name] = int(np.ceil(calls[name] * 1.3 * min_seconds / dt))
                dt = time_calls(fn, calls[name])
            samples[name].append(dt / calls[name])
    result = {}
    for name, per_call in samples.items():
        us = np.array(per_call) * 1e6
        result[name] = {'us_per_call': {'min': float(us.min()), 'median': float(np.median(us)),
                                        'max': float(us.max())},
                        'calls_per_repeat': calls[name], 'repeats': repeats}
    finite = {'B': all(bool(np.isfinite(a.get_params()).all()) for a in agents),
              'A': bool(torch.isfinite(eager.flat).all().item())}
    torch.cuda.synchronize()
    return {'obs_dim': D, 'act_dim': A, 'hidden': list(HIDDEN), 'act_rows': ACT_ROWS,
            'memory_records': MEMORY, 'sb_cycle': {'envs': envs, 'dataset_rows': rows,
                                                   'rollout_steps': ROLLOUT, 'train_steps': TRAIN,
                                                   'batch': SB_BATCH},
            'grid_max': 'min(CUs, 64) workgroups per branch',
            'params_finite_after': finite, 'legs': result}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--min-seconds', type=float, default=0.5)
    ap.add_argument('--envs', type=int, default=64)
    ap.add_argument('--rows', type=int, default=256)
    args = ap.parse_args()
    doc = {'workloads': {'optimize_49x10': run(args.repeats, args.min_seconds, args.envs,
                                               args.rows)}}
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(doc))


if __name__ == '__main__':
    main()
