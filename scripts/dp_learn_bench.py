"""What ``distribute`` costs ``learn`` on one GPU, and that it costs nothing
when it is not used.

Workload: 4096 envs of the config 2 shape (Optimize-v0 on gaussians_256x10,
41 -> 20), hidden (64, 64).  One call of a leg is one ``learn`` update: PPO2
with ``n_steps=128`` (4 epochs x 4 minibatches), A2C with ``n_steps=5``, DDPG
one cycle of 100 rollout + 50 train steps at batch 128 (``buffer_size=50000``);
``ddpg_train`` is that cycle's train phase alone (``DDPGAgent.train``).

Legs:
  A_*   ``learn`` without an exchange
  B_*   the same models after ``distribute(0, 1, collective=True)`` under the
        nccl backend: world 1 with the RCCL collective forced, so every step
        goes partial -> all-gather -> apply
  parent A_*   the A legs on another tree (``--parent-tree``: a checkout of the
        parent commit with its own built library), in a process of its own

Method: inside a process every leg is warmed up, then the legs
run alternately, ``--repeats`` repeats each, every repeat at least
``--min-seconds`` long and ended by a device synchronise; min / median / max
over the repeats.  The processes run parent, head_A (the A legs alone: the
parent's process with the head's code, no process group), head (A and B), parent,
so a drift of the machine shows as a difference between the two parent runs
and what the process group and the B models cost the A legs beside them shows
as head against head_A.

    python scripts/dp_learn_bench.py --parent-tree DIR --out profiles/r18_dp_learn.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

ROWS = 4096
HIDDEN = (64, 64)
ROLLOUT, TRAIN, BATCH, BUFFER = 100, 50, 128, 50000
SEED = 7


def build_legs(collective):
    import torch
    from custom_envs_amd import agents, ddpg
    from custom_envs_amd.vectorize.gpuvecenv import GPUVecEnv
    torch.cuda.set_device(0)
    if collective:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29517')
        dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))

    def env():
        e = GPUVecEnv(ROWS, data_set='gaussians_256x10', seed=0)
        e.reset()
        return e

    net = dict(net_arch=[dict(pi=list(HIDDEN), vf=list(HIDDEN))])

    def models():
        e = env()
        A = e.engine.act_dim
        return {
            'ppo2': agents.PPO2(agents.MlpPolicy, env(), n_steps=128, seed=SEED, policy_kwargs=net),
            'a2c': agents.A2C(agents.MlpPolicy, env(), n_steps=5, seed=SEED, policy_kwargs=net),
            'ddpg': agents.DDPG(ddpg.MlpPolicy, e, nb_rollout_steps=ROLLOUT, nb_train_steps=TRAIN,
                                batch_size=BATCH, buffer_size=BUFFER, seed=SEED,
                                action_noise=ddpg.NormalActionNoise(np.zeros(A), 0.1 * np.ones(A)),
                                policy_kwargs=dict(layers=list(HIDDEN)))}

    legs, keep = {}, []
    for prefix, dp in (('A', False), ('B', True)):
        if dp and not collective:
            continue
        group = models()
        keep.append(group)
        for name, model in group.items():
            if dp:
                model.distribute(0, 1, collective=True)

            def update(model=model):
                if model.rng.t + 4 * model.n_batch > 2 ** 32:
                    model.rng.t = 0
                model.learn(model.n_batch, reset_num_timesteps=False)
            legs['%s_%s' % (prefix, name)] = update
        d = group['ddpg']
        legs['%s_ddpg_train' % prefix] = \
            lambda d=d: d.agent.train(d.memory, TRAIN, BATCH, d.rng)
    return legs, keep


def time_calls(fn, calls):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def run_child(collective, repeats, min_seconds):
    import torch
    legs, keep = build_legs(collective)
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
    finite = all(bool(np.isfinite(m.get_parameters()).all()) for g in keep for m in g.values())
    n_params = {name: int(m.agent.n_params if name == 'ddpg' else m.policy.n_params)
                for name, m in keep[0].items()}
    if collective:
        torch.distributed.destroy_process_group()
    return {'device': torch.cuda.get_device_name(0), 'params_finite_after': finite,
            'n_params': n_params, 'legs': result}


def spawn(tree, collective, repeats, min_seconds):
    cmd = [sys.executable, os.path.abspath(__file__), '--child', '--tree', tree,
           '--repeats', str(repeats), '--min-seconds', str(min_seconds)]
    if collective:
        cmd.append('--collective')
    out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=900).stdout.decode()
    return json.loads(out.strip().splitlines()[-1])


def overlap(a, b):
    return bool(a['min'] <= b['max'] and b['min'] <= a['max'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--min-seconds', type=float, default=1.0)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--tree', default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument('--collective', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        sys.path.insert(0, os.path.abspath(args.tree))
        print(json.dumps(run_child(args.collective, args.repeats, args.min_seconds)))
        return
    doc = {'rows': ROWS, 'hidden': list(HIDDEN), 'nb_rollout_steps': ROLLOUT,
           'nb_train_steps': TRAIN, 'batch_size': BATCH, 'runs': []}
    order = [('head_A', ROOT, False), ('head', ROOT, True)]
    if args.parent_tree:
        order = [('parent', args.parent_tree, False)] + order + [('parent', args.parent_tree, False)]
    for label, tree, collective in order:
        doc['runs'].append(dict(tree=label, **spawn(tree, collective, args.repeats,
                                                    args.min_seconds)))
    head = next(r for r in doc['runs'] if r['tree'] == 'head')
    alone = next(r for r in doc['runs'] if r['tree'] == 'head_A')
    summary = {}
    for name in ('ppo2', 'a2c', 'ddpg', 'ddpg_train'):
        a, b = head['legs']['A_' + name]['us_per_call'], head['legs']['B_' + name]['us_per_call']
        row = {'A_median_us': a['median'], 'B_median_us': b['median'],
               'B_minus_A_us': b['median'] - a['median'], 'A_spread_us': a['max'] - a['min']}
        a = alone['legs']['A_' + name]['us_per_call']      # against the parent: the A legs alone
        row.update(A_alone_median_us=a['median'], A_alone_range_us=[a['min'], a['max']])
        parents = [r['legs']['A_' + name]['us_per_call'] for r in doc['runs'] if r['tree'] == 'parent']
        if parents:
            both = {'min': min(p['min'] for p in parents), 'max': max(p['max'] for p in parents)}
            row.update(parent_median_us=[p['median'] for p in parents], parent_range_us=both,
                       A_alone_range_overlaps_parent=overlap(a, both))
        summary[name] = row
    doc['summary'] = summary
    sys.path.insert(0, ROOT)
    from custom_envs_amd.learner import record_doubles
    n = head['n_params']['ddpg']
    doc['exchange_bytes_per_train_step'] = {
        'what': 'bytes every rank receives per DDPG train step: W records of 8 * '
                'record_doubles(n_params) B, at most W * (8 * n_params + 256)',
        'n_params': n, 'per_world': {str(w): w * 8 * record_doubles(n) for w in (1, 2, 4, 8)}}
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(doc['summary']))


if __name__ == '__main__':
    main()
