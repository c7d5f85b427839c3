"""``collect``: a K-step closed-loop rollout behind the vec-env surface.

What a PPO2 / A2C runner does per update -- K times (policy forward, env
step), storing observations, actions, values, neg-log-probs, rewards, dones
(run_multiagent_exp_single.py:37-49 through stable-baselines' runners) -- as
ONE engine call (``rollout_policy``) over device tensors.  ``GPUVecEnv.collect``
and the engine-backed ``OptVecEnv.collect`` are thin wrappers over
``run_collect``.

``collect_ddpg`` is the off-policy counterpart (``run_collect_ddpg``): K
times (``DDPGAgent.act``, env step) written straight into a
``ddpg.ReplayMemory``, the action noise either a tensor or formed inside the
act kernel from the counter-based generator (``noise=(action_noise,
device_rng)``).  The loop is issued from Python: the Python-issued
``[forward, step_device]`` loop measured 21.43 us per step against 21.11 us
for the single C call (README), so it has no C rollout entry.
"""
import numpy as np


def run_collect(engine, policy, n_steps, last_obs, noise, rows, normalizer=None):
    """Returns (result dict of device tensors, env fields).  ``last_obs``:
    the observation the env last returned (numpy or a device tensor).
    ``noise``: ``[K][rows][A]`` N(0,1) device tensor, None to draw it here
    (one ``torch.randn``), False for the deterministic policy, or a
    ``rng.DeviceRng``: the policy kernel forms draws ``t .. t + K - 1`` itself
    (no noise tensor exists) and the generator is advanced by K afterwards.
    ``normalizer``: a ``vecnormalize.VecNormalize``: a third launch per step
    normalises the step's observation and reward, the policy reads the
    normalised observations, and ``obs``, ``rewards``, ``last_obs`` and
    ``last_values`` are the normalised ones (the raw ones are added as
    ``original_obs`` and ``original_rewards``; the env fields stay raw)."""
    import torch
    from custom_envs_amd.rng import DeviceRng
    k = int(n_steps)
    if k < 1:
        raise ValueError('n_steps must be >= 1, got %d' % k)
    if last_obs is None:
        raise RuntimeError('collect() needs an observation to start from: call reset() first')
    dev = torch.device('cuda', policy.device)
    generated = isinstance(noise, DeviceRng)
    if torch.is_tensor(last_obs):
        obs0 = last_obs.to(dev).contiguous()
    else:
        obs0 = torch.from_numpy(np.ascontiguousarray(last_obs, dtype=np.float32)).to(dev)
    if noise is None:
        noise = torch.randn((k, rows, policy.act_dim), dtype=torch.float32, device=dev)
    elif noise is False:
        noise = None
    fields, rec, pfields, prec = engine.alloc_policy_rollout(k, policy)
    roll = None
    if normalizer is not None:
        vn = normalizer.normalizer
        roll = vn.begin_rollout(k, normalizer.training)
        raw0 = vn.original_obs
    # the tensors above were produced on torch's stream, the rollout runs on
    # the engine's: one synchronisation each way per K steps.  It stays with
    # generated noise too: the record buffers are zero-filled on torch's
    # stream, and their memory may be a block the learner's last update (on
    # torch's stream) still reads.
    torch.cuda.current_stream(dev).synchronize()
    if roll is None:
        engine.rollout_policy(k, policy, obs0, noise, fields, rec, pfields, prec)
    else:
        engine.rollout_policy(k, policy, roll.obs[0], noise, fields, rec, pfields, prec,
                              normalizer=roll)
    engine.wait()
    if generated:
        noise.advance(k)
    if roll is None:
        obs, rewards, last_obs = (torch.cat([obs0[None], fields['obs'][:k - 1]], dim=0),
                                  fields['reward'], fields['obs'][k - 1])
    else:
        obs, rewards, last_obs = roll.obs[:k].contiguous(), roll.rewards, roll.obs[k]
    last = policy.forward_device(last_obs)
    result = {
        'obs': obs,
        'actions': pfields['action'], 'env_actions': pfields['env_action'],
        'values': pfields['value'], 'neglogps': pfields['neglogp'],
        'rewards': rewards, 'dones': fields['done'],
        'last_obs': last_obs, 'last_values': last['value'],
    }
    if roll is not None:
        result['original_obs'] = torch.cat([raw0[None], fields['obs'][:k - 1]], dim=0)
        result['original_rewards'] = fields['reward']
        vn.end_rollout(roll, fields['obs'][k - 1], fields['reward'][k - 1])
    for name, value in fields.items():
        if name not in ('obs', 'reward', 'done', '_buffer'):
            result[name] = value
    return result, fields


def check_collect_ddpg(agent, memory, n_steps, noise, rows, obs_dim, act_dim):
    """Every argument check of ``run_collect_ddpg`` but the tensors' device
    (none needs a GPU).  Returns K."""
    import torch
    from custom_envs_amd.ddpg import DDPGAgent, ReplayMemory, check_tensor
    if not isinstance(agent, DDPGAgent):
        raise TypeError('agent must be a DDPGAgent')
    if not isinstance(memory, ReplayMemory):
        raise TypeError('memory must be a ReplayMemory')
    if (agent.obs_dim, agent.act_dim) != (obs_dim, act_dim):
        raise ValueError('the agent maps obs_dim %d -> act_dim %d, the engine\'s rows are %d -> %d'
                         % (agent.obs_dim, agent.act_dim, obs_dim, act_dim))
    if (memory.obs_dim, memory.act_dim) != (obs_dim, act_dim):
        raise ValueError('the memory holds obs_dim %d, act_dim %d, the engine\'s rows are %d -> %d'
                         % (memory.obs_dim, memory.act_dim, obs_dim, act_dim))
    if memory.rows != rows:
        raise ValueError('the memory takes %d rows per step, the engine writes %d'
                         % (memory.rows, rows))
    k = int(n_steps)
    if k < 1:
        raise ValueError('n_steps must be >= 1, got %d' % k)
    if isinstance(noise, tuple):
        from custom_envs_amd.ddpg import check_generated_noise
        check_generated_noise(noise, rows, act_dim, agent.WIDE)
        noise[1].check_draws(k)
    elif noise is not None:
        if not hasattr(noise, 'dim') or noise.dim() != 3 or noise.shape[0] < k:
            raise ValueError('noise must be [>= k][rows][A]; got shape %s for k = %d'
                             % (tuple(getattr(noise, 'shape', ())), k))
        check_tensor('noise', noise, torch.float32, (noise.shape[0], rows, act_dim))
    return k


def run_collect_ddpg(engine, agent, memory, n_steps, last_obs, noise, rows, obs_dim, act_dim,
                     stream, keep=()):
    """``n_steps`` closed-loop DDPG steps into the replay memory, all on
    ``stream`` (a ``torch.cuda.Stream`` the engine is put on for the call),
    with no host read and no allocation inside the loop.  Afterwards the
    engine is back on its OWN stream (``set_stream(0)``): it does not report
    the stream it had, so a caller who had put it on another one sets that
    again (the vec envs never do).  Per step, at the
    memory's next slot: the current observation is copied into ``obs0``;
    ``agent.act`` writes ``actions`` there and ``env_action`` into this call's
    record; the engine's ``step_device`` writes ``obs1``, ``rewards`` and
    ``dones`` there and its other fields into this call's records.

    The envs auto-reset: at a done row ``obs1`` is the reset observation, which
    the next step starts from and ``(1 - done)`` masks in ``y``.

    The engine writes ``obs1`` in place when every slot of it is 16-byte
    aligned (``rows * obs_dim`` a multiple of 4); otherwise through one aligned
    record and a copy, since some step kernels store the observation block in
    16-byte units.

    ``noise``: ``[>= K][rows][A]`` device tensor added to the actor's action
    (a Normal or Ornstein-Uhlenbeck process is state-independent), or None, or
    ``(action_noise, device_rng)``: the act kernel forms the noise itself, step
    ``j`` at draw ``device_rng.t + j``, and the generator is advanced by K
    afterwards.  An Ornstein-Uhlenbeck object's rows restart where the
    previous step's ``dones`` are set: the previous slot's, or for the call's
    first step the copy the object keeps of the last call's final ``dones``
    (no host read either way).
    ``keep``: memory fields (of ``obs1``, ``rewards``, ``dones``) to record per
    step as well, for a monitor.  Returns (result dict of ``[K]...`` device
    tensors: ``env_actions``, the engine's other fields, ``last_obs``; the kept
    records), synchronised."""
    import torch
    k = check_collect_ddpg(agent, memory, n_steps, noise, rows, obs_dim, act_dim)
    if last_obs is None:
        raise RuntimeError('collect_ddpg() needs an observation to start from: call reset() first')
    if getattr(engine, 'compact', False):
        raise ValueError('collect_ddpg needs the full output form (compact outputs are on)')
    dev = torch.device('cuda', agent.device)
    generated = isinstance(noise, tuple)
    ou = generated and hasattr(noise[0], 'ensure_state')
    if noise is not None and not generated:
        agent.check_device('noise', noise)
    agent.check_device('memory', memory.obs0)
    if ou:
        noise[0].ensure_state(rows, act_dim, dev)
    if torch.is_tensor(last_obs):
        cur = last_obs.to(dev).contiguous()
    else:
        cur = torch.from_numpy(np.ascontiguousarray(last_obs, dtype=np.float32)).to(dev)
    spec = engine.output_fields()
    other = [(name, dtype, r, tail) for name, dtype, r, tail in spec
             if name not in ('obs', 'reward', 'done')]
    records = {name: torch.empty((k, engine.num_envs * r) + tuple(tail), dtype=dtype, device=dev)
               for name, dtype, r, tail in other}
    env_actions = torch.empty((k, rows, act_dim), dtype=torch.float32, device=dev)
    source = {'obs1': memory.obs1, 'rewards': memory.rewards, 'dones': memory.dones}
    kept = {name: torch.empty((k, rows) + tuple(source[name].shape[1:]),
                              dtype=source[name].dtype, device=dev) for name in keep}
    in_place = (rows * obs_dim) % 4 == 0
    stage = None if in_place else torch.empty((rows, obs_dim), dtype=torch.float32, device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    engine.wait()
    engine.set_stream(stream.cuda_stream)
    prev_dones = noise[0].last_dones if ou else None
    try:
        with torch.cuda.stream(stream):
            for t in range(k):
                slot = memory.slot()
                obs0, obs1 = memory.obs0[slot], memory.obs1[slot]
                obs0.copy_(cur)
                act_out = {'action': memory.actions[slot], 'env_action': env_actions[t]}
                if generated:
                    agent.act(obs0, noise, out=act_out, stream=stream.cuda_stream,
                              t=noise[1].t + t, reset=prev_dones)
                    prev_dones = memory.dones[slot]
                else:
                    agent.act(obs0, None if noise is None else noise[t], out=act_out,
                              stream=stream.cuda_stream)
                out = {name: records[name][t] for name in records}
                out['obs'] = obs1 if in_place else stage
                out['reward'], out['done'] = memory.rewards[slot], memory.dones[slot]
                engine.step_device(env_actions[t], out)
                if not in_place:
                    obs1.copy_(stage)
                for name in keep:
                    kept[name][t].copy_(source[name][slot])
                cur = obs1
                memory.advance()
            if ou:
                noise[0].last_dones.copy_(prev_dones)
        stream.synchronize()
    finally:
        engine.set_stream(0)
    if generated:
        noise[1].advance(k)
    result = dict(records)
    result['env_actions'] = env_actions
    result['last_obs'] = cur.clone()     # not a view of a slot a later step overwrites
    return result, kept


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
