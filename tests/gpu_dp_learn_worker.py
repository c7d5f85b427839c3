"""One rank of the data-parallel training rehearsal on ONE GPU
(tests/test_gpu_dp_learn_ranks.py), or its one-process counterpart.

    RANK=r WORLD_SIZE=n MASTER_ADDR=127.0.0.1 MASTER_PORT=p \\
        python tests/gpu_dp_learn_worker.py OUT train ranks
    python tests/gpu_dp_learn_worker.py OUT train emulate WORLD
    RANK=r WORLD_SIZE=2 ... python tests/gpu_dp_learn_worker.py OUT ppo2|a2c|ddpg ranks
    python tests/gpu_dp_learn_worker.py OUT ppo2|a2c|ddpg single

``train``: every rank holds a ``DDPGAgent`` at ddpg_cases.CASES[2]'s
parameters with a ``GradientExchange`` (gloo carries the in-place all-gather
between processes on one device) and a memory filled with its shard of the
case's 70 rows, [33, 32(, 5)], and runs three ``train`` steps of 16 rows per
rank.  ``emulate``: one agent plays the ranks in turn, its indices from
``rng.replay_indices_numpy`` with the ranks' ``offset`` / ``total``.

``ppo2`` / ``a2c`` / ``ddpg`` ``ranks``: ``learn`` at world 2 on 4 + 2
two-class envs.  Run U is three updates straight; run R is two updates,
``save``, ``load`` + ``distribute`` and one more update on the same env.
``single``: one update of one model on all 6 envs.  Every process writes its
state to OUT(.rank<r>).npz.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

TRAIN_SHARDS = {2: [33, 32], 3: [33, 32, 5]}
TRAIN_BATCH, TRAIN_STEPS, TRAIN_SEED = 16, 3, 11
COUNTS = [4, 2]
ENV_SEED, MODEL_SEED = 21, 7
UPDATES = {'ppo2': 2, 'a2c': 2, 'ddpg': 3}       # before the save; one more follows


# ----------------------------------------------------------------------- train
def train_agent():
    import ddpg_cases as cases
    from custom_envs_amd.ddpg import DDPGAgent
    case = cases.CASES[2]
    inputs = cases.draw_case(case)
    _, D, hidden, A, _ = case
    agent = DDPGAgent(D, A, hidden, tau=0.01)
    agent.set_params(inputs['params'])
    agent.set_params(inputs['target_params'], target_only=True)
    return agent, inputs


def shard_memory(inputs, world, rank):
    import torch
    import ddpg_cases as cases
    from custom_envs_amd.ddpg import ReplayMemory
    shards = TRAIN_SHARDS[world]
    lo = sum(shards[:rank])
    n = shards[rank]
    memory = ReplayMemory(n, n, inputs['obs0'].shape[1], inputs['actions'].shape[1])
    for name in cases.FIELDS:
        getattr(memory, name).copy_(torch.from_numpy(
            np.ascontiguousarray(inputs[name][lo:lo + n])).cuda())
    memory.advance()
    return memory


def agent_state(agent, stats):
    import torch
    torch.cuda.synchronize()
    opt = agent.get_opt_state()
    return {'params': agent.get_params(), 'target': agent.get_params(target=True), 'm': opt['m'],
            'v': opt['v'], 'step': np.array(opt['step']), 'stats': stats.cpu().numpy()}


def main_train_ranks(out_path):
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    import torch
    import torch.distributed as dist
    from custom_envs_amd.distributed import GradientExchange
    from custom_envs_amd.rng import DeviceRng
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.cuda.set_device(0)
    agent, inputs = train_agent()
    ex = GradientExchange(agent, rank, world, collective=True)
    ex.broadcast_params(src=0)
    ex.broadcast_opt_state(src=0)
    stats = agent.train(shard_memory(inputs, world, rank), TRAIN_STEPS, TRAIN_BATCH,
                        DeviceRng(TRAIN_SEED))
    np.savez('%s.rank%d.npz' % (out_path, rank), **agent_state(agent, stats))
    dist.destroy_process_group()
    return 0


def main_train_emulate(out_path, world):
    import torch
    from custom_envs_amd import rng
    from custom_envs_amd.learner import N_STATS
    torch.cuda.set_device(0)
    agent, inputs = train_agent()
    memories = [shard_memory(inputs, world, r) for r in range(world)]
    B, total = TRAIN_BATCH, world * TRAIN_BATCH
    records = torch.zeros((world, agent.record_doubles), dtype=torch.float64, device='cuda')
    stats = torch.empty((TRAIN_STEPS, N_STATS), dtype=torch.float32, device='cuda')
    for s in range(TRAIN_STEPS):
        for r, memory in enumerate(memories):
            idx = rng.replay_indices_numpy(TRAIN_SEED, s, B, memory.size, offset=r * B, total=total)
            agent.partial(memory.as_batch(), torch.from_numpy(idx).cuda(), n_total=total,
                          out=records[r])
        agent.apply(records, total, stats=stats[s])
    np.savez(out_path, **agent_state(agent, stats))
    return 0


# ----------------------------------------------------------------------- learn
def make_env(rows, first):
    """``rows`` two-class envs, the global envs ``first ..`` (seeded by global
    index)."""
    import policy_cases as pc
    from custom_envs_amd.vectorize.gpuvecenv import GPUVecEnv
    features, targets = pc.rollout_dataset('lr_two_class_f64')
    return GPUVecEnv(rows, data_set=(features, targets), max_steps=4, seed=ENV_SEED + first)


def model_class(algo):
    from custom_envs_amd import agents
    return {'ppo2': agents.PPO2, 'a2c': agents.A2C, 'ddpg': agents.DDPG}[algo]


def make_model(algo, env):
    from custom_envs_amd import agents, ddpg
    if algo == 'ddpg':
        noise = ddpg.NormalActionNoise(np.zeros(20, np.float32), 0.1 * np.ones(20, np.float32))
        return agents.DDPG(ddpg.MlpPolicy, env, nb_rollout_steps=3, nb_train_steps=2, batch_size=4,
                           buffer_size=48, action_noise=noise, tau=0.01, actor_lr=1e-3,
                           critic_lr=1e-2, seed=MODEL_SEED, policy_kwargs=dict(layers=[32]))
    kw = dict(seed=MODEL_SEED, policy_kwargs=dict(net_arch=[dict(pi=[32], vf=[32])]))
    if algo == 'ppo2':
        return agents.PPO2(agents.MlpPolicy, env, n_steps=4, nminibatches=2, noptepochs=2,
                           learning_rate=1e-3, **kw)
    return agents.A2C(agents.MlpPolicy, env, n_steps=3, learning_rate=1e-3, **kw)


def record_first_rollout(env, algo, into):
    """Keep the first rollout's ``env_actions`` of ``env``."""
    name = 'collect_ddpg' if algo == 'ddpg' else 'collect'
    inner = getattr(env, name)

    def collect(*args, **kwargs):
        result = inner(*args, **kwargs)
        into.setdefault('env_actions', result['env_actions'].cpu().numpy().copy())
        return result
    setattr(env, name, collect)


def model_state(model, prefix):
    import torch
    torch.cuda.synchronize()
    opt = model.get_opt_state()
    out = {prefix + 'params': model.get_parameters(),
           prefix + 'num_timesteps': np.array(model.num_timesteps),
           prefix + 'opt_step': np.array(opt['step'])}
    for name, value in opt.items():
        if name != 'step':
            out[prefix + 'opt_' + name] = value
    if hasattr(model, 'agent'):
        out[prefix + 'target'] = model.get_parameters(target=True)
    return out


def after_first_update(into):
    def callback(locals_, _globals):
        if locals_['update'] == 1:
            into['params_update1'] = locals_['self'].get_parameters()
        return True
    return callback


def main_learn_ranks(out_path, algo):
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    import torch
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.cuda.set_device(0)
    assert world == len(COUNTS)
    first, n = sum(COUNTS[:rank]), UPDATES[algo]
    out = {}

    # run U: n + 1 updates straight
    env = make_env(COUNTS[rank], first)
    record_first_rollout(env, algo, out)
    model = make_model(algo, env)
    model.distribute(rank, world, counts=COUNTS, collective=True)
    assert model.rng.row_offset == first
    model.learn((n + 1) * model.n_batch, callback=after_first_update(out))
    out.update(model_state(model, 'u_'))
    env.close()

    # run R: n updates, save, load + distribute, one more on the same env
    env = make_env(COUNTS[rank], first)
    model = make_model(algo, env)
    model.distribute(rank, world, counts=COUNTS, collective=True)
    model.learn(n * model.n_batch)
    out.update(model_state(model, 'a_'))
    if algo == 'ddpg':      # the memory is this rank's own: every rank saves and loads its own
        path = '%s.save%d.npz' % (out_path, rank)
        model.save(path, memory=True)
    else:                   # the replicas are identical: rank 1's file serves both
        path = '%s.save.npz' % out_path
        if rank == 1:
            model.save(path)
    dist.barrier()
    resumed = model_class(algo).load(path, env=env)
    assert resumed.num_timesteps == n * model.n_batch
    resumed.distribute(rank, world, counts=COUNTS, collective=True)
    resumed.learn(resumed.n_batch, reset_num_timesteps=False)
    out.update(model_state(resumed, 'r_'))
    env.close()
    np.savez('%s.rank%d.npz' % (out_path, rank), **out)
    dist.destroy_process_group()
    return 0


def main_learn_single(out_path, algo):
    import torch
    torch.cuda.set_device(0)
    out = {}
    env = make_env(sum(COUNTS), 0)
    record_first_rollout(env, algo, out)
    model = make_model(algo, env)
    model.learn(model.n_batch, callback=after_first_update(out))
    out.update(model_state(model, 'u_'))
    env.close()
    np.savez(out_path, **out)
    return 0


if __name__ == '__main__':
    out_path, what, mode = sys.argv[1:4]
    if what == 'train':
        sys.exit(main_train_emulate(out_path, int(sys.argv[4])) if mode == 'emulate'
                 else main_train_ranks(out_path))
    sys.exit(main_learn_single(out_path, what) if mode == 'single'
             else main_learn_ranks(out_path, what))
