"""Closed-loop rollouts with the policy on the device: what the policy between
env steps costs, and what one `rollout_policy` call makes of it.

Workloads: config 2 (Optimize-v0, 256 x 10, two classes, float64, 4096 envs)
and config 5 (MultiOptLRs 'func4', 1024 envs x 4 agents); the policy is
stable-baselines' MlpPolicy shape, hidden (64, 64); K = 128 steps per call.

Legs (each K steps per call, everything on one stream):
  A  the form a caller has without this feature: the same network in eager
     torch (torch.nn.Linear / tanh, torch.randn drawn per step, clamp, the
     neg-log-prob) + step_device per step
  B  MlpPolicy.forward_device + step_device per step from Python
  C  rollout_policy: one foreign call for the K steps
  D  for context, no policy: D_rollout = the open-loop rollout_device (fixed
     actions), D_step = step_device per step (fixed actions)

Method: every leg is warmed up, then the legs run alternately, five repeats
each, every repeat at least a second long and ended by a device synchronise;
min / median / max over the repeats.

    python scripts/policy_rollout_bench.py --out profiles/r07_policy_rollout.json
    rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- \
        python scripts/policy_rollout_bench.py --trace-leg-c
    python scripts/policy_rollout_bench.py --summarize-trace DIR/run_kernel_stats.csv \
        --out profiles/r07_policy_rollout_kernels.json
"""
import argparse
import csv
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


class EagerPolicy:
    """Leg A: the network as a caller writes it in eager torch."""

    def __init__(self, params, n_hidden, low, high, device):
        import torch

        def net(prefix):
            layers = []
            for i in range(n_hidden):
                layers += [self._linear(params['%s/w%d' % (prefix, i)], params['%s/b%d' % (prefix, i)], device),
                           torch.nn.Tanh()]
            layers.append(self._linear(params[prefix + '/w_out'], params[prefix + '/b_out'], device))
            return torch.nn.Sequential(*layers)

        self.pi, self.vf = net('pi'), net('vf')
        self.logstd = torch.from_numpy(params['logstd']).to(device)
        self.low, self.high = low, high
        self.const = 0.5 * self.logstd.numel() * float(np.log(2 * np.pi))

    @staticmethod
    def _linear(w, b, device):
        import torch
        lin = torch.nn.Linear(w.shape[0], w.shape[1])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(w.T.copy()))
            lin.bias.copy_(torch.from_numpy(b))
        return lin.to(device)

    def __call__(self, obs):
        import torch
        with torch.no_grad():
            mean = self.pi(obs)
            value = self.vf(obs)[:, 0]
            noise = torch.randn_like(mean)
            action = mean + torch.exp(self.logstd) * noise
            env_action = torch.clamp(action, self.low, self.high)
            neglogp = 0.5 * torch.sum(noise * noise, dim=1) + self.logstd.sum() + self.const
        return action, env_action.contiguous(), neglogp, value


def make_workload(config):
    from custom_envs_amd.policy import MlpPolicy
    if config == 2:
        from custom_envs_amd.engine import OptimizeEngine
        from custom_envs_amd.envs.optimize import resolve_dataset
        features, targets = resolve_dataset('gaussians_256x10', None)
        eng = OptimizeEngine(features, targets, num_envs=4096)
        eng.seed(0)
        rows, D, A, envs, low, high = 4096, eng.obs_dim, eng.act_dim, 4096, -1e3, 1e3
    else:
        from custom_envs_amd.multi_engine import MultiOptEngine
        eng = MultiOptEngine(1024, 'func4')
        rows, D, A, envs, low, high = eng.rows, 3 * eng.max_history, 1, 1024, -1e3, 1e4
    policy = MlpPolicy(D, A, HIDDEN, low=low, high=high)
    params = draw_params(policy.params_layout(), np.random.RandomState(7))
    policy.set_params(params)
    return eng, policy, params, rows, D, A, envs, low, high


def build_legs(config, stream):
    """name -> callable running K steps (stream-ordered, no sync inside)."""
    import torch
    eng, policy, params, rows, D, A, envs, low, high = make_workload(config)
    eng.set_stream(stream.cuda_stream)
    dev = torch.device('cuda', 0)
    out = eng.alloc_device_outputs()
    eng.reset_device(out)
    fields, rec, pfields, prec = eng.alloc_policy_rollout(K, policy)
    noise = torch.randn((K, rows, A), dtype=torch.float32, device=dev)
    eager = EagerPolicy(params, len(HIDDEN), low, high, dev)
    pout = policy.alloc_outputs(rows)
    fixed = (0.01 * torch.randn((K, rows, A), dtype=torch.float32, device=dev)).contiguous()

    def leg_a():
        for _ in range(K):
            _, env_action, _, _ = eager(out['obs'])
            eng.step_device(env_action, out)

    def leg_b():
        for t in range(K):
            policy.forward_device(out['obs'], noise[t], out=pout)
            eng.step_device(pout['env_action'], out)

    def leg_c():
        eng.rollout_policy(K, policy, out['obs'], noise, fields, rec, pfields, prec)
        out['obs'].copy_(fields['obs'][K - 1])

    def leg_d_rollout():
        eng.rollout_device(K, fixed, fields, rec)

    def leg_d_step():
        for t in range(K):
            eng.step_device(fixed[t], out)

    legs = {'A_eager_torch_policy': leg_a, 'B_forward_device_per_step': leg_b,
            'C_rollout_policy': leg_c, 'D_rollout_device_open_loop': leg_d_rollout,
            'D_step_device_no_policy': leg_d_step}
    return legs, envs, rows, (eng, policy, out)


def time_calls(fn, calls, stream):
    stream.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    stream.synchronize()
    return time.perf_counter() - t0


def run_config(config, repeats, min_seconds):
    import torch
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        legs, envs, rows, keep = build_legs(config, stream)
        calls = {}
        for name, fn in legs.items():             # warm up, then size a repeat to >= min_seconds
            time_calls(fn, 3, stream)
            n = 4
            while True:
                dt = time_calls(fn, n, stream)
                if dt >= 0.25 * min_seconds:
                    break
                n *= 2
            calls[name] = max(1, int(np.ceil(n * min_seconds * 1.3 / dt)))
        samples = {name: [] for name in legs}
        for _ in range(repeats):                  # the legs alternately
            for name, fn in legs.items():
                dt = time_calls(fn, calls[name], stream)
                while dt < min_seconds:            # a short repeat is discarded and redone longer
                    calls[name] = int(np.ceil(calls[name] * 1.3 * min_seconds / dt))
                    dt = time_calls(fn, calls[name], stream)
                samples[name].append(dt / (calls[name] * K))
        finite = bool(torch.isfinite(keep[2]['obs']).all())
    result = {}
    for name, per_step in samples.items():
        us = np.array(per_step) * 1e6
        result[name] = {
            'us_per_step': {'min': float(us.min()), 'median': float(np.median(us)), 'max': float(us.max())},
            'env_steps_per_s': {'min': float(envs / us.max() * 1e6), 'median': float(envs / np.median(us) * 1e6),
                                'max': float(envs / us.min() * 1e6)},
            'calls_per_repeat': calls[name], 'repeats': repeats}
    assert finite
    return {'envs': envs, 'policy_rows': rows, 'k': K, 'hidden': list(HIDDEN), 'legs': result}


def trace_leg_c():
    """Leg C alone, a few calls: the workload of the kernel-trace run."""
    import torch
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for config in (2, 5):
            legs, _, _, keep = build_legs(config, stream)
            time_calls(legs['C_rollout_policy'], 20, stream)
            print('config', config, 'traced 20 calls of', K, 'steps')


def summarize_trace(path, out):
    rows = list(csv.DictReader(open(path)))
    keep = []
    for r in rows:
        name = r.get('Name', '')
        if any(s in name for s in ('policy_', 'optimize_lr', 'multi_step', 'multi_reset')):
            keep.append({'kernel': name, 'calls': int(r['Calls']),
                         'average_us': float(r['AverageNs']) / 1e3, 'min_us': float(r['MinNs']) / 1e3,
                         'max_us': float(r['MaxNs']) / 1e3, 'total_ms': float(r['TotalDurationNs']) / 1e6})
    doc = {'source': 'rocprofv3 --kernel-trace --stats, leg C (rollout_policy) alone, configs 2 and 5, '
                     '20 calls of 128 steps each',
           'kernels': keep}
    with open(out, 'w') as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--min-seconds', type=float, default=1.0)
    ap.add_argument('--configs', default='2,5')
    ap.add_argument('--trace-leg-c', action='store_true')
    ap.add_argument('--summarize-trace', default=None)
    args = ap.parse_args()
    if args.summarize_trace:
        return summarize_trace(args.summarize_trace, args.out)
    if args.trace_leg_c:
        return trace_leg_c()
    doc = {'workloads': {'config%d' % c: run_config(c, args.repeats, args.min_seconds)
                         for c in (int(v) for v in args.configs.split(','))}}
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(doc))


if __name__ == '__main__':
    main()
