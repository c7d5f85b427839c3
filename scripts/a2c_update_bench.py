"""The A2C update after a 5-step rollout: the device-side learner
(custom_envs_amd/a2c.py) against the same work in eager torch on the same GPU,
in the same process.

Workloads: the policy shapes of configs 2 and 5 (4096 rows x 41 -> 20, and
'func4', 1024 envs x 4 agents = 4096 rows x 15 -> 1), hidden (64, 64),
K = 5 steps, one gradient step on all 20 480 rows.  The update does not depend
on what produced the rollout, so for legs A - C the rollout is synthetic, in
collect's layout (strided policy and env records): N(0,1) observations,
actions sampled from the policy itself, random rewards, an episode end at
step 3 of every 8th row.

Legs:
  A  the update in eager torch: the returns loop over K, forward, A2C loss,
     autograd backward, clip_grad_norm_, RMSProp (TF's form, as tensors), and
     the flat parameters handed to MlpPolicy.set_params
  B  learner.returns + learner.flatten + learner.step
  C  learner.update, on the records in place
  D  GPUVecEnv.collect(5) + learner.update, closed loop, 4096 envs of the
     two-class shape (config2 only), reported as env-steps/s as well

Method: every leg is warmed up, then the legs run alternately, `repeats`
repeats each, every repeat at least `min-seconds` long and ended by a device
synchronise; min / median / max over the repeats.

    python scripts/a2c_update_bench.py --out profiles/r10_a2c_update.json
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

K = 5
ROWS = 4096
HIDDEN = (64, 64)
SHAPES = {'config2': (41, 20), 'config5_func4': (15, 1)}
HYPER = dict(gamma=0.99, ent_coef=0.01, vf_coef=0.25, max_grad_norm=0.5, lr=7e-4, alpha=0.99,
             eps=1e-5)


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
    """Leg A as a caller writes it without the feature."""

    def __init__(self, policy, params, device):
        import torch
        self.policy = policy
        self.layout = policy.params_layout()
        self.flat = torch.zeros(policy.n_params, dtype=torch.float32, device=device, requires_grad=True)
        with torch.no_grad():
            for name, (off, shape) in self.layout.items():
                self.flat[off:off + int(np.prod(shape))] = torch.from_numpy(params[name].reshape(-1)).to(device)
        self.ms = torch.ones_like(self.flat)
        self.n_hidden = len(policy.hidden)
        self.A = policy.act_dim

    def views(self):
        return {name: self.flat[off:off + int(np.prod(shape))].view(shape)
                for name, (off, shape) in self.layout.items()}

    def returns(self, rewards, dones, last_values):
        import torch
        ret = torch.empty_like(rewards)
        carry = last_values
        for t in range(rewards.shape[0] - 1, -1, -1):
            carry = rewards[t] + HYPER['gamma'] * carry * (1.0 - dones[t].float())
            ret[t] = carry
        return ret

    def update(self, result):
        import torch
        ret = self.returns(result['rewards'], result['dones'], result['last_values']).reshape(-1)
        total = ret.numel()
        obs = result['obs'].reshape(total, -1)
        act = result['actions'].reshape(total, -1)
        adv = ret - result['values'].reshape(-1)
        p = self.views()

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
        pg = (adv * nlp).mean()
        vf = ((vpred - ret) ** 2).mean()
        loss = pg - HYPER['ent_coef'] * entropy + HYPER['vf_coef'] * vf
        self.flat.grad = None
        loss.backward()
        torch.nn.utils.clip_grad_norm_([self.flat], HYPER['max_grad_norm'])
        with torch.no_grad():
            g = self.flat.grad
            self.ms.mul_(HYPER['alpha']).addcmul_(g, g, value=1.0 - HYPER['alpha'])
            self.flat.addcdiv_(g, (self.ms + HYPER['eps']).sqrt_(), value=-HYPER['lr'])
            self.policy.set_params(self.flat.detach())
        return loss


def build_legs(shape):
    import torch
    from custom_envs_amd.a2c import A2CLearner
    from custom_envs_amd.policy import MlpPolicy
    D, A = SHAPES[shape]
    dev = torch.device('cuda', 0)

    def make(low=None, high=None):
        policy = MlpPolicy(D, A, HIDDEN, low=low, high=high)
        params = draw_params(policy.params_layout(), np.random.RandomState(7))
        policy.set_params(params)
        return policy, params

    policy, params = make()
    learners = {name: A2CLearner(make()[0], **HYPER) for name in ('B', 'C')}
    eager_policy, _ = make()
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
    dones[3, ::8] = 1
    last_values = torch.randn(ROWS, dtype=torch.float32, device=dev, generator=gen)
    result = {'obs': obs, 'actions': pfields['action'], 'values': pfields['value'],
              'rewards': rewards, 'dones': dones, 'last_values': last_values}
    torch.cuda.synchronize()

    def leg_b():
        learner = learners['B']
        learner.step(learner.flatten(result, learner.returns(result)))

    legs = {
        'A_eager_update': lambda: eager.update(result),
        'B_returns_flatten_step': leg_b,
        'C_update_in_place': lambda: learners['C'].update(result),
    }
    keep = [policy, eager_policy, learners]
    if shape == 'config2':
        from custom_envs_amd.vectorize.gpuvecenv import GPUVecEnv
        env = GPUVecEnv(ROWS, data_set='gaussians_256x10', seed=0)
        assert (env.engine.obs_dim, env.engine.act_dim) == (D, A)
        loop_policy, _ = make(low=-1e3, high=1e3)
        loop_learner = A2CLearner(loop_policy, **HYPER)
        env.reset()

        def leg_d():
            loop_learner.update(env.collect(loop_policy, K))

        legs['D_collect_update_closed_loop'] = leg_d
        keep += [env, loop_policy, loop_learner]
        learners = dict(learners, D=loop_learner)
    return legs, learners, keep


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
    legs, learners, keep = build_legs(shape)
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
    finite = {name: bool(np.isfinite(learner.get_params()).all()) for name, learner in learners.items()}
    result = {}
    for name, per_call in samples.items():
        us = np.array(per_call) * 1e6
        result[name] = {'us_per_call': {'min': float(us.min()), 'median': float(np.median(us)),
                                        'max': float(us.max())},
                        'calls_per_repeat': calls[name], 'repeats': repeats}
        if name.startswith('D_'):
            result[name]['env_steps_per_s'] = {
                'min': K * ROWS / (us.max() * 1e-6), 'median': K * ROWS / (float(np.median(us)) * 1e-6),
                'max': K * ROWS / (us.min() * 1e-6)}
    D, A = SHAPES[shape]
    torch.cuda.synchronize()
    return {'rows': ROWS, 'k': K, 'obs_dim': D, 'act_dim': A, 'hidden': list(HIDDEN),
            'update_rows': K * ROWS, 'params_finite_after': finite, 'legs': result}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--min-seconds', type=float, default=1.0)
    ap.add_argument('--shapes', default=','.join(SHAPES))
    args = ap.parse_args()
    doc = {'workloads': {s: run_shape(s, args.repeats, args.min_seconds) for s in args.shapes.split(',')}}
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(doc))


if __name__ == '__main__':
    main()
