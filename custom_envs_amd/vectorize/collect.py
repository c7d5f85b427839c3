"""``collect``: a K-step closed-loop rollout behind the vec-env surface.

What a PPO2 / A2C runner does per update -- K times (policy forward, env
step), storing observations, actions, values, neg-log-probs, rewards, dones
(run_multiagent_exp_single.py:37-49 through stable-baselines' runners) -- as
ONE engine call (``rollout_policy``) over device tensors.  ``GPUVecEnv.collect``
and the engine-backed ``OptVecEnv.collect`` are thin wrappers over
``run_collect``.
"""
import numpy as np


def run_collect(engine, policy, n_steps, last_obs, noise, rows):
    """Returns (result dict of device tensors, env fields).  ``last_obs``:
    the observation the env last returned (numpy or a device tensor).
    ``noise``: ``[K][rows][A]`` N(0,1) device tensor, None to draw it here
    (one ``torch.randn``), or False for the deterministic policy."""
    import torch
    k = int(n_steps)
    if k < 1:
        raise ValueError('n_steps must be >= 1, got %d' % k)
    if last_obs is None:
        raise RuntimeError('collect() needs an observation to start from: call reset() first')
    dev = torch.device('cuda', policy.device)
    if torch.is_tensor(last_obs):
        obs0 = last_obs.to(dev).contiguous()
    else:
        obs0 = torch.from_numpy(np.ascontiguousarray(last_obs, dtype=np.float32)).to(dev)
    if noise is None:
        noise = torch.randn((k, rows, policy.act_dim), dtype=torch.float32, device=dev)
    elif noise is False:
        noise = None
    fields, rec, pfields, prec = engine.alloc_policy_rollout(k, policy)
    # the tensors above were produced on torch's stream, the rollout runs on
    # the engine's: one synchronisation each way per K steps
    torch.cuda.current_stream(dev).synchronize()
    engine.rollout_policy(k, policy, obs0, noise, fields, rec, pfields, prec)
    engine.wait()
    last = policy.forward_device(fields['obs'][k - 1])
    result = {
        'obs': torch.cat([obs0[None], fields['obs'][:k - 1]], dim=0),
        'actions': pfields['action'], 'env_actions': pfields['env_action'],
        'values': pfields['value'], 'neglogps': pfields['neglogp'],
        'rewards': fields['reward'], 'dones': fields['done'],
        'last_obs': fields['obs'][k - 1], 'last_values': last['value'],
    }
    for name, value in fields.items():
        if name not in ('obs', 'reward', 'done', '_buffer'):
            result[name] = value
    return result, fields


def host_records(fields):
    """The K env records on the host with ONE device-to-host copy: numpy
    views of a copy of the rollout buffer, laid out as the device views."""
    host = fields['_buffer'].cpu()
    out = {}
    for name, v in fields.items():
        if name == '_buffer':
            continue
        out[name] = host.view(v.dtype).as_strided(v.shape, v.stride(), v.storage_offset()).numpy()
    return out
