"""Write tests/golden/point_env_walls_{dense,dense_squared,sparse}.npz and point_env_momentum_{...}.npz: trajectories of the
REFERENCE's MetaPointEnvWalls and MetaPointEnvMomentum (envs/point_envs/point_env_2d_walls.py, point_env_2d_momentum.py), which pin
the NumPy restatement tests/point_family_checks.py:env_step, the classes of promp_amd/envs/point_env.py and through them the device.

    python tools/gen_point_family_golden.py /path/to/the/reference/checkout

The reference is imported with a stand-in for gym's Box, the way oracle/gen_golden.py:gen_point_env does.  Needs nothing but NumPy.

Each fixture: seed (np.random.seed in front of the reference's sample_tasks), tasks, start states, policy-scale actions, next
observations, rewards, the wrapper's scale (0: the bare class was driven) and the action box.
  walls    normalize(MetaPointEnvWalls) for dense and dense_squared; the bare class for sparse, whose None outside the reward radius
           the wrapper cannot carry: recorded as 0.0 with the mask reward_is_none.  After reset() the state is set to radius 0.9
           (even tasks) or 1.9 (odd tasks), at the gap's angle or 2 rad away from it, and the actions push outwards.  events [B][T]:
           0 none, 1 wall 1 threw the point back, 2 wall 1 passed through the gap, 3 / 4 the same at wall 2.  All of 1 .. 4 occur.
  momentum normalize(MetaPointEnvMomentum) for dense and sparse, the bare class for dense_squared; some actions beyond the box."""
import contextlib
import io
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
SEEDS = dict(dense=41, dense_squared=42, sparse=43)


class Box(object):
    def __init__(self, low, high, shape=None, dtype=None):
        self.low = np.broadcast_to(np.asarray(low, dtype=np.float64), shape if shape is not None else np.shape(low)).copy()
        self.high = np.broadcast_to(np.asarray(high, dtype=np.float64), shape if shape is not None else np.shape(high)).copy()
        self.shape = self.low.shape


def import_reference(path):
    sys.path.insert(0, path)
    for name in ('gym', 'gym.core', 'gym.spaces', 'gym.envs', 'gym.envs.mujoco', 'rand_param_envs', 'rand_param_envs.gym',
                 'rand_param_envs.gym.spaces'):
        mod = types.ModuleType(name)
        mod.Box, mod.Env, mod.MujocoEnv, mod.__path__ = Box, object, object, []
        sys.modules.setdefault(name, mod)
    sys.modules['gym'].spaces = sys.modules['gym.spaces']
    sys.modules['gym'].core = sys.modules['gym.core']
    sys.modules['rand_param_envs'].gym = sys.modules['rand_param_envs.gym']
    sys.modules['rand_param_envs.gym'].spaces = sys.modules['rand_param_envs.gym.spaces']
    from meta_policy_search.envs.point_envs.point_env_2d_walls import MetaPointEnvWalls
    from meta_policy_search.envs.point_envs.point_env_2d_momentum import MetaPointEnvMomentum
    from meta_policy_search.envs.normalized_env import normalize
    return MetaPointEnvWalls, MetaPointEnvMomentum, normalize


def quiet(make):
    with contextlib.redirect_stdout(io.StringIO()):      # (the classes print their reward type)
        return make()


def gen_walls(Walls, normalize, reward_type, n_tasks=8, T=30):
    rng = np.random.RandomState(SEEDS[reward_type])
    bare = quiet(lambda: Walls(reward_type=reward_type))
    wrapped = reward_type != 'sparse'
    env = normalize(bare) if wrapped else bare
    scale = float(env._normalization_scale) if wrapped else 0.0
    seed = int(rng.randint(1 << 30))
    np.random.seed(seed)
    tasks = env.sample_tasks(n_tasks)
    start, actions, nxt = np.zeros((n_tasks, 2)), np.zeros((n_tasks, T, 2)), np.zeros((n_tasks, T, 2))
    rew, none, events = np.zeros((n_tasks, T)), np.zeros((n_tasks, T), bool), np.zeros((n_tasks, T), np.int32)
    for b, task in enumerate(tasks):
        env.set_task(task)
        env.reset()
        wall = 1 + b % 2
        gap = task['gap_%d' % wall]
        angle = np.arctan2(gap[1], gap[0]) + (0.0 if (b // 2) % 2 == 0 else 2.0)
        bare._state = (wall - 0.1) * np.array([np.cos(angle), np.sin(angle)])
        start[b] = bare._state
        # policy-scale actions pushing outwards (so that the walls are met again and again), some beyond the wrapper's box
        push = (6.0 if wrapped else 0.12) * np.array([np.cos(angle), np.sin(angle)])
        actions[b] = push + (5.0 if wrapped else 0.1) * rng.randn(T, 2)
        for t in range(T):
            before = bare._state.copy()
            low, high = bare.action_space.low, bare.action_space.high
            e = np.clip(low + (actions[b, t] + scale) * (high - low) / (2 * scale), low, high) if wrapped else actions[b, t]
            moved = before + np.clip(e, -0.2, 0.2)                  # (the state the walls look at: point_env_2d_walls.py:37)
            o, r, done, info = env.step(actions[b, t])
            assert done is False and info == {}
            nxt[b, t], none[b, t], rew[b, t] = o, r is None, 0.0 if r is None else r
            thrown = not np.array_equal(o, moved)
            if np.linalg.norm(before) < 1 and np.linalg.norm(moved) > 1:
                events[b, t] = 1 if thrown else 2
            elif np.linalg.norm(before) < 2 and np.linalg.norm(moved) > 2:
                events[b, t] = 3 if thrown else 4
            else:
                assert not thrown
    counts = [int(np.sum(events == k)) for k in range(5)]
    assert all(counts[1:]), counts
    if reward_type == 'sparse':
        assert np.any(rew != 0) and none.any() and not none.all()
    np.savez(os.path.join(GOLDEN, 'point_env_walls_%s.npz' % reward_type), seed=seed,
             goals=np.array([t['goal'] for t in tasks], np.float64), gaps_1=np.array([t['gap_1'] for t in tasks]),
             gaps_2=np.array([t['gap_2'] for t in tasks]), start=start, actions=actions, next_observations=nxt, rewards=rew,
             reward_is_none=none, events=events, normalization_scale=scale, action_low=bare.action_space.low,
             action_high=bare.action_space.high, sparse_reward_radius=float(bare.sparse_reward_radius))
    print('wrote point_env_walls_%s.npz  events 1..4: %s  None rewards: %d  nonzero rewards: %d of %d' % (
        reward_type, counts[1:], int(none.sum()), int(np.count_nonzero(rew)), rew.size))


def gen_momentum(Momentum, normalize, reward_type, n_tasks=6, T=40):
    rng = np.random.RandomState(SEEDS[reward_type] + 100)
    bare = quiet(lambda: Momentum(reward_type=reward_type))
    wrapped = reward_type != 'dense_squared'
    env = normalize(bare) if wrapped else bare
    scale = float(env._normalization_scale) if wrapped else 0.0
    seed = int(rng.randint(1 << 30))
    np.random.seed(seed)
    tasks = env.sample_tasks(n_tasks)
    start, actions, nxt = np.zeros((n_tasks, 4)), np.zeros((n_tasks, T, 2)), np.zeros((n_tasks, T, 4))
    rew = np.zeros((n_tasks, T))
    for b, goal in enumerate(tasks):
        env.set_task(goal)
        start[b] = env.reset()
        # accelerate towards the goal (so that the sparse reward fires) or away from it, plus noise beyond the box in some rows
        drift = np.sign(goal) * (1.0 if b % 2 == 0 else -0.5)
        actions[b] = (drift * 2.0 + 6.0 * rng.randn(T, 2)) if wrapped else (drift * 0.02 + 0.08 * rng.randn(T, 2))
        for t in range(T):
            o, r, done, info = env.step(actions[b, t])
            assert done is False and info == {}
            nxt[b, t], rew[b, t] = o, r
    box = scale if wrapped else 0.1
    assert (np.abs(actions) > box).any()
    if wrapped:
        assert (np.abs(actions) > 10).any()
    if reward_type == 'sparse':
        assert 0 < np.count_nonzero(rew) < rew.size
    np.savez(os.path.join(GOLDEN, 'point_env_momentum_%s.npz' % reward_type), seed=seed, goals=np.asarray(tasks, np.float64),
             start=start, actions=actions, next_observations=nxt, rewards=rew, normalization_scale=scale,
             action_low=bare.action_space.low, action_high=bare.action_space.high,
             sparse_reward_radius=float(bare.sparse_reward_radius))
    print('wrote point_env_momentum_%s.npz  nonzero rewards: %d of %d' % (reward_type, int(np.count_nonzero(rew)), rew.size))


if __name__ == '__main__':
    Walls, Momentum, normalize = import_reference(sys.argv[1])
    for reward_type in ('dense', 'dense_squared', 'sparse'):
        gen_walls(Walls, normalize, reward_type)
        gen_momentum(Momentum, normalize, reward_type)
