"""DDPG's two loops -- collecting into the replay memory and the train step --
on the device-side learner (custom_envs_amd/ddpg.py) against the same work in
eager torch on the same GPU, in the same process.

Workload: 4096 envs of the config 2 shape (Optimize-v0 on gaussians_256x10,
41 -> 20), hidden (64, 64), a replay memory of 16 env steps (65 536 records).

Legs:
  A_collect  10 env steps in eager torch: clip, the relu actor, tanh, noise,
             clip, scale as tensor ops, ``step_device``, and the records copied
             into the memory's slot
  B_collect  ``GPUVecEnv.collect_ddpg`` of 10 steps
  A_train_N  one train step at batch N in eager torch: gather by index, the
             target networks, both losses, autograd, Adam on both blocks (as
             tensors), the soft update
  B_train_N  ``ReplayMemory.sample`` + ``DDPGAgent.step`` at batch N
for N = 128 (stable-baselines' batch) and N = 4096.  ``sb_cycle`` is derived
from the medians: stable-baselines' cycle of 100 rollout steps and 50 train
steps at batch 128.

Method: every leg is warmed up, then the legs run alternately, `repeats`
repeats each, every repeat at least `min-seconds` long and ended by a device
synchronise; min / median / max over the repeats.

    python scripts/ddpg_update_bench.py --out profiles/r13_ddpg_update.json
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

ROWS = 4096
HIDDEN = (64, 64)
COLLECT_K = 10
MEMORY_STEPS = 16
BATCHES = (128, 4096)
HYPER = dict(gamma=0.99, tau=0.001, actor_lr=1e-4, critic_lr=1e-3)
SCALE = 0.01


class EagerDDPG:
    """Legs A as a caller writes them without the feature."""

    def __init__(self, layout, flat, n_actor, device):
        import torch
        self.layout, self.n_actor = layout, n_actor
        self.flat = torch.from_numpy(flat.copy()).to(device).requires_grad_(True)
        self.target = self.flat.detach().clone()
        self.m = torch.zeros_like(self.target)
        self.v = torch.zeros_like(self.target)
        self.lr = torch.cat([torch.full((n_actor,), HYPER['actor_lr']),
                             torch.full((flat.size - n_actor,), HYPER['critic_lr'])]).to(device)
        self.t = 0

    def views(self, flat):
        return {name: flat[off:off + int(np.prod(shape))].view(shape)
                for name, (off, shape) in self.layout.items()}

    @staticmethod
    def actor(p, o):
        import torch
        x = o
        for i in range(len(HIDDEN)):
            x = torch.relu(x @ p['actor/w%d' % i] + p['actor/b%d' % i])
        return torch.tanh(x @ p['actor/w_out'] + p['actor/b_out'])

    @staticmethod
    def critic(p, o, a):
        import torch
        x = o
        for i in range(len(HIDDEN)):
            x = torch.relu(x @ p['critic/w%d' % i] + p['critic/b%d' % i])
            if i == 0:
                x = torch.cat([x, a], dim=1)
        return (x @ p['critic/w_out'] + p['critic/b_out'])[:, 0]

    def act(self, obs, noise):
        import torch
        with torch.no_grad():
            a = self.actor(self.views(self.flat), obs.clamp(-5.0, 5.0))
            a = (a + noise).clamp_(-1.0, 1.0)
            return a, a * SCALE

    def train(self, memory, idx):
        import torch
        idx = idx.long()
        o0 = memory.obs0[idx].clamp(-5.0, 5.0)
        o1 = memory.obs1[idx].clamp(-5.0, 5.0)
        act, rew = memory.actions[idx], memory.rewards[idx]
        nonterminal = 1.0 - memory.dones[idx].float()
        with torch.no_grad():
            tp = self.views(self.target)
            y = rew + HYPER['gamma'] * nonterminal * self.critic(tp, o1, self.actor(tp, o1))
        p = self.views(self.flat)
        critic_loss = ((self.critic(p, o0, act) - y) ** 2).mean()
        frozen = self.views(self.flat.detach())       # the actor's loss moves the actor only
        actor_loss = -self.critic(frozen, o0, self.actor(p, o0)).mean()
        self.flat.grad = None
        (critic_loss + actor_loss).backward()
        with torch.no_grad():
            g = self.flat.grad
            self.t += 1
            corr = float(np.sqrt(1.0 - 0.999 ** self.t) / (1.0 - 0.9 ** self.t))
            self.m.mul_(0.9).add_(g, alpha=0.1)
            self.v.mul_(0.999).addcmul_(g, g, value=0.001)
            self.flat.sub_(self.lr * corr * self.m / (self.v.sqrt() + 1e-8))
            self.target.mul_(1.0 - HYPER['tau']).add_(self.flat, alpha=HYPER['tau'])
        return critic_loss


def build_legs():
    import torch
    from custom_envs_amd import ddpg
    from custom_envs_amd.vectorize.gpuvecenv import GPUVecEnv
    dev = torch.device('cuda', 0)
    envs = {name: GPUVecEnv(ROWS, data_set='gaussians_256x10', seed=0) for name in ('A', 'B')}
    D, A = envs['A'].engine.obs_dim, envs['A'].engine.act_dim
    flat = ddpg.init_params_numpy(D, A, HIDDEN, seed=7)
    agent = ddpg.DDPGAgent(D, A, HIDDEN, scale=SCALE, **HYPER)
    agent.set_params(flat)
    eager = EagerDDPG(agent.params_layout(), flat, agent.n_actor, dev)
    memories = {name: ddpg.ReplayMemory(MEMORY_STEPS * ROWS, ROWS, D, A) for name in ('A', 'B')}
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1)
    noise = 0.1 * torch.randn((COLLECT_K, ROWS, A), dtype=torch.float32, device=dev, generator=gen)
    for env in envs.values():
        env.reset()

    # leg A's loop on the engine's device outputs, on torch's stream
    eng, mem_a = envs['A'].engine, memories['A']
    out = eng.alloc_device_outputs()
    eng.reset_device(out)
    eng.wait()
    side = torch.cuda.Stream(dev)     # one stream for torch's ops and the engine's, as leg B has
    eng.set_stream(side.cuda_stream)
    state = {'obs': out['obs'].clone()}
    torch.cuda.synchronize()

    def collect_a():
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for t in range(COLLECT_K):
                slot = mem_a.slot()
                action, env_action = eager.act(state['obs'], noise[t])
                mem_a.obs0[slot].copy_(state['obs'])
                mem_a.actions[slot].copy_(action)
                eng.step_device(env_action, out)
                mem_a.obs1[slot].copy_(out['obs'])
                mem_a.rewards[slot].copy_(out['reward'])
                mem_a.dones[slot].copy_(out['done'])
                state['obs'].copy_(out['obs'])
                mem_a.advance()
        side.synchronize()

    def collect_b():
        envs['B'].collect_ddpg(agent, memories['B'], COLLECT_K, noise)

    for _ in range(2):          # both memories full before a train step samples them
        collect_a()
        collect_b()
    torch.cuda.synchronize()
    legs = {'A_collect': collect_a, 'B_collect': collect_b}
    for n in BATCHES:
        legs['A_train_%d' % n] = (
            lambda n=n: eager.train(mem_a, mem_a.sample(n, generator=gen)))
        legs['B_train_%d' % n] = (
            lambda n=n: agent.step(memories['B'].as_batch(), memories['B'].sample(n, generator=gen)))
    return legs, agent, eager, [envs, memories, out, noise]


def time_calls(fn, calls):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def run(repeats, min_seconds):
    import torch
    legs, agent, eager, keep = build_legs()
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
        if name.endswith('_collect'):
            result[name]['us_per_env_step'] = float(np.median(us)) / COLLECT_K
            result[name]['us_per_row_step'] = float(np.median(us)) / COLLECT_K / ROWS
    cycle = {}
    for leg in 'AB':                          # derived: 100 rollout steps + 50 train steps
        step_us = result[leg + '_collect']['us_per_env_step']
        train_us = result['%s_train_128' % leg]['us_per_call']['median']
        cycle[leg + '_ms'] = (100 * step_us + 50 * train_us) / 1e3
    finite = {'B': bool(np.isfinite(agent.get_params()).all()),
              'A': bool(torch.isfinite(eager.flat).all().item())}
    torch.cuda.synchronize()
    return {'rows': ROWS, 'obs_dim': agent.obs_dim, 'act_dim': agent.act_dim,
            'hidden': list(HIDDEN), 'collect_k': COLLECT_K, 'memory_records': MEMORY_STEPS * ROWS,
            'params_finite_after': finite, 'legs': result,
            'sb_cycle_100_rollout_50_train_derived': cycle}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--min-seconds', type=float, default=1.0)
    args = ap.parse_args()
    doc = {'workloads': {'config2': run(args.repeats, args.min_seconds)}}
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(doc))


if __name__ == '__main__':
    main()
