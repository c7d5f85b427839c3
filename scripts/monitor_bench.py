"""What a monitored ``collect`` costs: the host ``VecMonitor`` against the
device monitor (``utils_logging.DeviceVecMonitor``) against no monitor.

Workloads, K = 128 steps per ``collect``, hidden (64, 64), deterministic policy:
  optimize   config 2 (Optimize-v0, 256 x 10, two classes, float64) at 4096
             envs, ``max_steps`` 40, info keywords objective / accuracy
  func4      1024 MultiOptLRs-v0 ``func4`` envs (4 agents each), ``max_batches``
             40, the scripts' seven info keywords
each with ``paths=None`` and with per-env ``.mon.csv`` files (chunk_size 5, the
scripts' default) in a temporary directory.

Rows:  A  the host ``VecMonitor`` path (``host_records`` + K Python passes)
       B  the device monitor
       C  no monitor
One child process per (workload, files, row), each under its own time limit;
a child warms up, then times five ``collect`` calls, each ended by a device
synchronise and each preceded, outside the timed region, by a full
``gc.collect()``: every monitored row allocates one dict per finished episode,
and a cyclic collection of the whole heap (torch's objects included) that
happens to start inside a repeat costs more than the monitor does.  The parent
never opens the GPU, and stops at the first child that fails.  Medians and min-max ranges go to ``--out`` with B - C and A - C,
the bytes the device monitor drained per collect and the bytes
``host_records`` moves.

    python scripts/monitor_bench.py --out profiles/r19_monitor.json
    rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- \\
        python scripts/monitor_bench.py --trace
    python scripts/monitor_bench.py --summarize-trace DIR/run_kernel_stats.csv \\
        --out profiles/r19_monitor_kernels.json
"""
import argparse
import csv
import functools
import gc
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

K = 128
HIDDEN = (64, 64)
SIZES = {'optimize': 4096, 'func4': 1024}
MULTI_KEYS = ('loss', 'actions_mean', 'weights_mean', 'actions_std', 'states_mean', 'grads_mean',
              'grad_diff')
CHUNK = 5


def build(workload, envs, row, directory):
    """(env, policy, bytes host_records moves per collect)."""
    from custom_envs_amd.agents import init_params_numpy
    from custom_envs_amd.policy import MlpPolicy
    paths = None if directory is None else [os.path.join(directory, str(i)) for i in range(envs)]
    if workload == 'optimize':
        from custom_envs_amd.vectorize.gpuvecenv import GPUVecEnv
        monitor = None if row == 'C' else (paths, {
            'info_keywords': ('objective', 'accuracy'), 'chunk_size': CHUNK, 'device': row == 'B'})
        env = GPUVecEnv(envs, data_set='gaussians_256x10', max_steps=40, seed=0, monitor=monitor)
        eng, rows = env.engine, envs
        obs_dim, act_dim = eng.obs_dim, eng.act_dim
        space = env.single_action_space
    else:
        from custom_envs_amd.core import make
        from custom_envs_amd.utils.utils_logging import Monitor
        from custom_envs_amd.vectorize.optvecenv import OptVecEnv
        target = functools.partial(make, 'MultiOptLRs-v0', problem='func4', max_batches=40)
        fns = [target if row == 'C' else functools.partial(
            Monitor, target, None if paths is None else paths[i], info_keywords=MULTI_KEYS,
            chunk_size=CHUNK) for i in range(envs)]
        env = OptVecEnv(fns, device_monitor=row == 'B')
        eng, rows = env._engine, env._engine.rows
        obs_dim, act_dim = 3 * eng.max_history, 1
        space = env.action_space
    policy = MlpPolicy(obs_dim, act_dim, HIDDEN, low=space.low.reshape(-1),
                       high=space.high.reshape(-1))
    flat = init_params_numpy(policy.params_layout(), 0)
    policy.set_params(flat)
    return env, policy, K * eng.alloc_rollout(1)[1]


def child(workload, envs, row, files, repeats, warmup):
    import torch
    with tempfile.TemporaryDirectory() as tmp:
        env, policy, host_bytes = build(workload, envs, row, tmp if files else None)
        env.reset()
        times, drained = [], []
        for i in range(warmup + repeats):
            before = getattr(env.monitor, 'drained_bytes', 0)
            gc.collect()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            env.collect(policy, K, noise=False)
            torch.cuda.synchronize()
            if i >= warmup:
                times.append(time.perf_counter() - t0)
                drained.append(getattr(env.monitor, 'drained_bytes', 0) - before)
        episodes = None if env.monitor is None else sum(
            len(r) for r in env.env_method('get_episode_rewards'))
        env.close()
    print(json.dumps({'ms': [1e3 * t for t in times], 'drained_bytes': drained,
                      'host_records_bytes': host_bytes, 'episodes': episodes}))


def summary(ms):
    return {'median_ms': float(np.median(ms)), 'min_ms': float(min(ms)), 'max_ms': float(max(ms))}


def parent(args):
    doc = {'k': K, 'hidden': list(HIDDEN), 'chunk_size': CHUNK, 'repeats': args.repeats,
           'warmup': args.warmup, 'rows': {'A': 'host VecMonitor', 'B': 'device monitor',
                                           'C': 'no monitor'}, 'configurations': []}
    for workload in args.workloads.split(','):
        envs = args.envs or SIZES[workload]
        for files in (False, True):
            entry = {'workload': workload, 'envs': envs, 'files': files}
            for row in 'CBA':
                cmd = [sys.executable, os.path.abspath(__file__), '--child', workload, row,
                       '--envs', str(envs), '--repeats', str(args.repeats),
                       '--warmup', str(args.warmup)] + (['--files'] if files else [])
                proc = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.child_seconds)
                if proc.returncode != 0:
                    print('child failed (%d): %s' % (proc.returncode, ' '.join(cmd)), file=sys.stderr)
                    return proc.returncode or 1
                got = json.loads(proc.stdout.decode().strip().splitlines()[-1])
                entry[row] = dict(summary(got['ms']), ms=got['ms'], episodes=got['episodes'])
                if row == 'B':
                    entry['drained_bytes_per_collect'] = float(np.median(got['drained_bytes']))
                entry['host_records_bytes_per_collect'] = got['host_records_bytes']
            a, b, c = (entry[r] for r in 'ABC')
            entry['A_minus_C_ms'] = a['median_ms'] - c['median_ms']
            entry['B_minus_C_ms'] = b['median_ms'] - c['median_ms']
            entry['B_range_below_A_range'] = b['max_ms'] < a['min_ms']
            doc['configurations'].append(entry)
            print(json.dumps({k: v for k, v in entry.items() if k not in 'ABC'}), flush=True)
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(doc))
    return 0


def trace():
    """The device monitor alone on both workloads, a few collects: the
    workload of the kernel-trace run."""
    import torch
    for workload in ('optimize', 'func4'):
        env, policy, _ = build(workload, SIZES[workload], 'B', None)
        env.reset()
        for _ in range(4):
            env.collect(policy, K, noise=False)
        torch.cuda.synchronize()
        env.close()
        print(workload, 'traced 4 collects of', K, 'steps')


def summarize_trace(path, out):
    keep = []
    for r in csv.DictReader(open(path)):
        name = r.get('Name', '')
        if 'monitor_' in name:
            keep.append({'kernel': name, 'calls': int(r['Calls']),
                         'average_us': float(r['AverageNs']) / 1e3, 'min_us': float(r['MinNs']) / 1e3,
                         'max_us': float(r['MaxNs']) / 1e3, 'total_ms': float(r['TotalDurationNs']) / 1e6})
    doc = {'source': 'rocprofv3 --kernel-trace --stats, 4 collects of 128 steps with the device '
                     'monitor at 4096 config-2 envs and at 1024 func4 envs',
           'kernels': keep}
    with open(out, 'w') as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--envs', type=int, default=None)
    ap.add_argument('--workloads', default='optimize,func4')
    ap.add_argument('--child-seconds', type=float, default=240.0,
                    help='the time limit of each child process')
    ap.add_argument('--child', nargs=2, metavar=('WORKLOAD', 'ROW'), default=None)
    ap.add_argument('--files', action='store_true')
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--summarize-trace', default=None)
    args = ap.parse_args()
    if args.summarize_trace:
        return summarize_trace(args.summarize_trace, args.out)
    if args.trace:
        return trace()
    if args.child:
        return child(args.child[0], args.envs or SIZES[args.child[0]], args.child[1], args.files,
                     args.repeats, args.warmup)
    return parent(args)


if __name__ == '__main__':
    sys.exit(main() or 0)
