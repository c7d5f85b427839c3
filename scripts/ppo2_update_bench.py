"""The PPO2 update after a rollout: the device-side learner (custom_envs_amd/ppo2.py)
against the same work in eager torch on the same GPU, in the same process.

Workloads: the policy shapes of configs 2 and 5 (4096 rows x 41 -> 20, and
'func4', 1024 envs x 4 agents = 4096 rows x 15 -> 1), hidden (64, 64),
K = 128 steps, nminibatches = 4, noptepochs = 4.  The update does not depend on
what produced the rollout, so the rollout is synthetic: N(0,1) observations,
actions sampled from the policy itself, random rewards, an episode end every
40 steps.

Legs:
  A  GAE as an eager-torch reverse loop over K
  B  learner.gae (one launch)
  C  one eager-torch minibatch step: forward, PPO2 loss, autograd backward,
     clip_grad_norm_, Adam (TF epsilon placement, as tensors), and the flat
     parameters handed to MlpPolicy.set_params
  D  learner.step (one call)
  E  a full update (GAE + 4 epochs x 4 minibatches, one randperm per epoch),
     eager and learner.update

Method: every leg is warmed up, then the legs run alternately, `repeats`
repeats each, every repeat at least `min-seconds` long and ended by a device
synchronise; min / median / max over the repeats.

    python scripts/ppo2_update_bench.py --out profiles/r08_ppo2_update.json
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
ROWS = 4096
HIDDEN = (64, 64)
NMINIBATCHES = 4
NOPTEPOCHS = 4
SHAPES = {'config2': (41, 20), 'config5_func4': (15, 1)}
HYPER = dict(gamma=0.99, lam=0.95, cliprange=0.2, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5,
             lr=2.5e-4)


def draw_params(layout, rs):
    params = {}
    for name, (_, shape) in layout.items():
        if name == 'logstd':
            value = np.full(shape, -0.5)
        elif len(shape) == 2:
            value = rs.normal(0, 1, shape) / np.sqrt(shape[0])
        else:
            value = 0.1 * rs.normal(0, 1, shape)
        params[name] = value.astype(np.float32)
    return params


class EagerLearner:
    """Legs A, C and E as a caller writes them without the feature."""

    def __init__(self, policy, params, device):
        import torch
        self.policy = policy
        self.layout = policy.params_layout()
        self.flat = torch.zeros(policy.n_params, dtype=torch.float32, device=device, requires_grad=True)
        with torch.no_grad():
            for name, (off, shape) in self.layout.items():
                self.flat[off:off + int(np.prod(shape))] = torch.from_numpy(params[name].reshape(-1)).to(device)
        self.m = torch.zeros_like(self.flat)
        self.v = torch.zeros_like(self.flat)
        self.t = 0
        self.n_hidden = len(policy.hidden)
        self.A = policy.act_dim

    def views(self):
        return {name: self.flat[off:off + int(np.prod(shape))].view(shape)
                for name, (off, shape) in self.layout.items()}

    def gae(self, rewards, values, dones, last_values):
        import torch
        adv = torch.empty_like(rewards)
        carry = torch.zeros_like(last_values)
        for t in range(rewards.shape[0] - 1, -1, -1):
            nt = 1.0 - dones[t].float()
            v_next = last_values if t == rewards.shape[0] - 1 else values[t + 1]
            delta = rewards[t] + HYPER['gamma'] * v_next * nt - values[t]
            carry = delta + HYPER['gamma'] * HYPER['lam'] * nt * carry
            adv[t] = carry
        return adv, adv + values

    def step(self, batch, idx):
        import torch
        p = self.views()
        obs, act = batch['obs'][idx], batch['actions'][idx]
        adv, ret = batch['advantages'][idx], batch['returns'][idx]
        old_nlp, old_v = batch['neglogps'][idx], batch['values'][idx]

        def mlp(net):
            x = obs
            for i in range(self.n_hidden):
                x = torch.tanh(x @ p['%s/w%d' % (net, i)] + p['%s/b%d' % (net, i)])
            return x @ p[net + '/w_out'] + p[net + '/b_out']

        mean, vpred = mlp('pi'), mlp('vf')[:, 0]
        logstd = p['logstd']
        nlp = (0.5 * (((act - mean) / torch.exp(logstd)) ** 2).sum(1) + logstd.sum()
               + 0.5 * self.A * float(np.log(2 * np.pi)))
        entropy = (logstd + 0.5 * float(np.log(2 * np.pi * np.e))).sum()
        adv = (adv - adv.mean()) / (adv.std(unbiased=False) + 1e-8)
        ratio = torch.exp(old_nlp - nlp)
        c = HYPER['cliprange']
        pg = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - c, 1 + c)).mean()
        vclip = old_v + torch.clamp(vpred - old_v, -c, c)
        vf = 0.5 * torch.max((vpred - ret) ** 2, (vclip - ret) ** 2).mean()
        loss = pg - HYPER['ent_coef'] * entropy + HYPER['vf_coef'] * vf
        self.flat.grad = None
        loss.backward()
        torch.nn.utils.clip_grad_norm_([self.flat], HYPER['max_grad_norm'])
        with torch.no_grad():
            self.t += 1
            g = self.flat.grad
            self.m.mul_(0.9).add_(g, alpha=0.1)
            self.v.mul_(0.999).addcmul_(g, g, value=0.001)
            lr_t = HYPER['lr'] * np.sqrt(1 - 0.999 ** self.t) / (1 - 0.9 ** self.t)
            self.flat.addcdiv_(self.m, self.v.sqrt().add_(1e-5), value=-lr_t)
            self.policy.set_params(self.flat.detach())
        return loss

    def update(self, result):
        import torch
        adv, ret = self.gae(result['rewards'], result['values'], result['dones'], result['last_values'])
        total = adv.numel()
        batch = {'obs': result['obs'].reshape(total, -1), 'actions': result['actions'].reshape(total, -1),
                 'advantages': adv.reshape(-1), 'returns': ret.reshape(-1),
                 'neglogps': result['neglogps'].reshape(-1), 'values': result['values'].reshape(-1)}
        size = total // NMINIBATCHES
        for _ in range(NOPTEPOCHS):
            perm = torch.randperm(total, device=adv.device)
            for b in range(NMINIBATCHES):
                self.step(batch, perm[b * size:(b + 1) * size])


def build_legs(shape):
    import torch
    from custom_envs_amd.policy import MlpPolicy
    from custom_envs_amd.ppo2 import PPO2Learner
    D, A = SHAPES[shape]
    dev = torch.device('cuda', 0)
    rs = np.random.RandomState(7)
    policy = MlpPolicy(D, A, HIDDEN)
    params = draw_params(policy.params_layout(), rs)
    policy.set_params(params)
    learner = PPO2Learner(policy, **HYPER)
    eager_policy = MlpPolicy(D, A, HIDDEN)
    eager_policy.set_params(params)
    eager = EagerLearner(eager_policy, params, dev)

    # a synthetic rollout in collect's layout: strided policy and env records
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1)
    pfields, _ = policy.alloc_outputs(ROWS, K)
    obs = torch.randn((K, ROWS, D), dtype=torch.float32, device=dev, generator=gen)
    noise = torch.randn((K, ROWS, A), dtype=torch.float32, device=dev, generator=gen)
    for t in range(K):
        policy.forward_device(obs[t], noise[t], out={n: pfields[n][t] for n in
                                                     ('action', 'env_action', 'neglogp', 'value')})
    rec = torch.zeros((K, 2 * ROWS + 64), dtype=torch.float32, device=dev)    # padded records
    rewards = rec[:, :ROWS]
    rewards.copy_(torch.randn((K, ROWS), dtype=torch.float32, device=dev, generator=gen))
    dones = torch.zeros((K, ROWS + 64), dtype=torch.uint8, device=dev)[:, :ROWS]
    dones[39::40] = 1
    last_values = torch.randn(ROWS, dtype=torch.float32, device=dev, generator=gen)
    result = {'obs': obs, 'actions': pfields['action'], 'values': pfields['value'],
              'neglogps': pfields['neglogp'], 'rewards': rewards, 'dones': dones,
              'last_values': last_values}
    adv, ret = learner.gae(result)
    batch = learner.flatten(result, adv, ret)
    total = K * ROWS
    perm = torch.randperm(total, dtype=torch.int32, device=dev, generator=gen)
    idx = perm[:total // NMINIBATCHES].contiguous()
    idx64 = idx.long()
    torch.cuda.synchronize()

    legs = {
        'A_eager_gae': lambda: eager.gae(rewards, pfields['value'], dones, last_values),
        'B_learner_gae': lambda: learner.gae(result),
        'C_eager_minibatch_step': lambda: eager.step(batch, idx64),
        'D_learner_step': lambda: learner.step(batch, idx),
        'E_eager_update': lambda: eager.update(result),
        'E_learner_update': lambda: learner.update(result, NOPTEPOCHS, NMINIBATCHES, generator=gen),
    }
    return legs, (policy, learner, eager_policy)


def time_calls(fn, calls):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def run_shape(shape, repeats, min_seconds):
    import torch
    legs, keep = build_legs(shape)
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
    assert bool(torch.isfinite(keep[1].get_params(out=torch.empty(keep[0].n_params, device='cuda'))).all())
    result = {}
    for name, per_call in samples.items():
        us = np.array(per_call) * 1e6
        result[name] = {'us_per_call': {'min': float(us.min()), 'median': float(np.median(us)),
                                        'max': float(us.max())},
                        'calls_per_repeat': calls[name], 'repeats': repeats}
    D, A = SHAPES[shape]
    return {'rows': ROWS, 'k': K, 'obs_dim': D, 'act_dim': A, 'hidden': list(HIDDEN),
            'nminibatches': NMINIBATCHES, 'noptepochs': NOPTEPOCHS,
            'minibatch_rows': K * ROWS // NMINIBATCHES, 'legs': result}


def trace_leg_d():
    """learner.step alone, a few calls: the workload of a kernel-trace run."""
    for shape in SHAPES:
        legs, _ = build_legs(shape)
        time_calls(legs['D_learner_step'], 20)
        print(shape, 'traced 20 calls of learner.step')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--min-seconds', type=float, default=1.0)
    ap.add_argument('--shapes', default=','.join(SHAPES))
    ap.add_argument('--trace-leg-d', action='store_true')
    args = ap.parse_args()
    if args.trace_leg_d:
        return trace_leg_d()
    doc = {'workloads': {s: run_shape(s, args.repeats, args.min_seconds) for s in args.shapes.split(',')}}
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(doc))


if __name__ == '__main__':
    main()
