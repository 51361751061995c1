"""CPU side of the terminating point-mass environments (tests/point_collect_checks.py): MetaPointEnv and MetaPointEnvV2 against the
reference's trajectories, the float64 restatement of the goal step against the same fixtures, the collection oracle against the
package's own MetaSampler, and the soundness of every case test_gpu_point_collect.py runs (events, margins) on the oracle alone."""
import copy

import numpy as np
import pytest

from oracle import policy as op
from tests import point_collect_checks as pc
from tests.test_gpu_point_collect import FIXED, GOAL


@pytest.mark.parametrize('name', ['origin', 'goal'])
def test_classes_reproduce_the_reference(name):
    g = pc.load_fixture(name)
    n, T = g['actions'].shape[:2]
    assert g['dones'].sum() >= 10 and (~g['dones']).sum() >= 10
    for b in range(n):
        env, bare = pc.make_env(name, float(g['normalization_scales'][b]))
        assert env.sample_tasks(3) is not None and np.array_equal(bare.action_space.high, g['action_high'])
        env.set_task({} if name == 'origin' else g['tasks'][b])
        env.reset()
        bare._state = g['start'][b].copy()
        for t in range(T):
            o, r, d, info = env.step(g['actions'][b, t])
            assert np.array_equal(o, g['next_observations'][b, t]) and r == g['rewards'][b, t] and info == {}
            assert isinstance(d, bool) and d == bool(g['dones'][b, t]), (b, t)
        assert np.array_equal(np.asarray(env.get_task() if name == 'goal' else g['tasks'][b]), g['tasks'][b])


def test_class_conventions():
    from promp_amd.envs import point_env
    np.random.seed(3)
    origin, goal = point_env.MetaPointEnv(), point_env.MetaPointEnvV2()
    assert origin.sample_tasks(4) == [{}] * 4 and origin.get_task() == {}
    assert np.all(np.abs(np.array([origin.reset() for _ in range(50)])) <= 2) and np.array_equal(goal.reset(), np.zeros(2))
    tasks = goal.sample_tasks(5)
    assert tasks.shape == (5, 2) and np.all(np.abs(tasks) <= 2)
    goal.set_task(tasks[2])
    assert np.array_equal(goal.get_task(), tasks[2])                   # (the reference reads an attribute it never sets)
    assert point_env.make_point_env('origin').__class__ is point_env.MetaPointEnv
    assert point_env.make_point_env('goal').__class__ is point_env.MetaPointEnvV2
    assert not hasattr(origin, 'reward_type')
    # the quirk: V2's done looks at the origin, not at the goal
    goal.set_task(np.array([0.005, 0.005]))
    goal.reset()
    assert goal.step(np.array([0.004, 0.004]))[2] is True
    goal._state = np.array([1.0, 1.0])
    goal.set_task(np.array([1.001, 1.001]))
    assert goal.step(np.array([0.001, 0.001]))[2] is False


@pytest.mark.parametrize('name', ['origin', 'goal'])
def test_goal_step_restates_the_reference(name):
    g = pc.load_fixture(name)
    n, T = g['actions'].shape[:2]
    for b in range(n):
        state = g['start'][b][None, :]
        for t in range(T):
            state, r, d, _ = pc.goal_step(state, g['actions'][b, t][None, :], g['tasks'][b], float(g['normalization_scales'][b]))
            assert np.array_equal(state[0], g['next_observations'][b, t]) and r[0] == g['rewards'][b, t] and d[0] == g['dones'][b, t]


class _StubPolicy(object):
    """get_actions of the oracle's policy on the oracle's noise table, one row per call"""

    def __init__(self, c):
        self.c, self.calls = c, 0

    def get_actions(self, obs_by_task):
        c = self.c
        obs32 = np.concatenate([np.asarray(o, np.float32) for o in obs_by_task])
        mean, act = pc.policy_actions(c['spec'], c['th'], obs32, c['z'][self.calls], c['B'])
        self.calls += 1
        act = act.astype(np.float32).astype(np.float64).reshape(c['M'], c['B'], 2)       # what the environment consumes
        infos = [[dict(mean=m) for m in mean[i * c['B']:(i + 1) * c['B']]] for i in range(c['M'])]
        return list(act), infos


@pytest.mark.parametrize('dims,scale,rollouts,origin', [((2, 3, 12, (32, 32)), 10, None, False), ((3, 2, 8, (32, 32)), 0, 4, True)])
def test_oracle_is_the_host_sampler(dims, scale, rollouts, origin):
    """the package's MetaSampler driving the NumPy class, resets served from the start table: the same paths in the same order, the
    same stop step, the same rows"""
    from promp_amd.envs import point_env
    from promp_amd.envs.normalized_env import normalize
    from promp_amd.samplers.meta_sampler import MetaSampler
    M, B, T, hidden = dims
    c = pc.goal_case(M, B, T, hidden, scale, 'host', 0, 0, data_seed=1, rollouts=rollouts, origin=origin)
    o = pc.case_oracle(c)

    base = point_env.MetaPointEnv if origin else point_env.MetaPointEnvV2

    class TableEnv(base):
        index, steps = 0, 0

        def reset(self):
            # (an episode that ends with the last vectorised step the bound allows is reset once more; nobody steps it again)
            self._state = c['start'][self.steps, self.index].copy() if self.steps < c['S'] else np.zeros(2)
            return self._state.copy()

        def step(self, action):
            self.steps += 1
            return base.step(self, action)

    bare = TableEnv()
    env = normalize(bare) if scale > 0 else bare
    policy = _StubPolicy(c)
    sampler = MetaSampler(env, policy, rollouts or B, M, T, envs_per_task=B)
    for e, one in enumerate(sampler.vec_env.envs):
        (one.wrapped_env if scale > 0 else one).index = e
    sampler.vec_env.set_tasks([{}] * M if origin else list(c['tasks']))
    paths = sampler.obtain_samples()
    t = o['tables']
    assert t is not None and policy.calls == t['stop'] + 1 and sampler.total_samples == c['total']
    assert [len(paths[i]) for i in range(M)] == np.diff(t['tpo']).tolist()
    flat = [p for i in range(M) for p in paths[i]]
    assert [len(p['rewards']) for p in flat] == t['len'].tolist() and sum(t['len']) == t['rows']
    assert np.array_equal(np.concatenate([p['observations'] for p in flat]).astype(np.float32), pc.gather(o['obs'], t))
    assert np.array_equal(np.concatenate([p['rewards'] for p in flat]), pc.gather(o['rew'], t))
    assert np.array_equal(np.concatenate([p['actions'] for p in flat]), pc.gather(o['act'], t).astype(np.float32).astype(np.float64))
    assert len(set(t['len'])) > 1 and (t['len'] < T).any()


def test_tables_of_ties_and_shortfalls():
    """hand-made end_len: two episodes end at the stop step (both count), a task that finishes nothing, one step short; and the
    inputs that realise it on the device do so on the oracle"""
    end_len = pc.HAND_END_LEN
    t = pc.tables_of(end_len, 2, 3, 9)
    for k, v in pc.HAND_TABLES.items():
        assert np.array_equal(t[k], v), k
    assert pc.tables_of(end_len[:3], 2, 3, 9) is None and pc.tables_of(end_len, 2, 3, 24) is None
    assert pc.tables_of(end_len, 2, 3, 1)['tpo'].tolist() == [0, 0, 1] and pc.tables_of(end_len, 2, 3, 5)['tpo'].tolist() == [0, 1, 3]
    assert pc.tables_of(end_len, 2, 3, 8)['stop'] == 2 and pc.tables_of(end_len, 2, 3, 23)['stop'] == 4
    pc.hand_case()


def test_gpu_cases_cover_the_required_events():
    wanted = set().union(*(set(c[6]) for c in GOAL))
    assert wanted == set(pc.EVENTS)
    assert {c[3] for c in GOAL} == {0, 1} and {c[5] for c in GOAL} == {True, False} and {c[2] for c in GOAL} == {'host', 'device'}
    assert {c[4] for c in GOAL if c[2] == 'device'} == {pc.SEED31, pc.SEED64} and {c[1] for c in GOAL} == {0, 10}
    assert any(c[8] is not None and c[8] > c[0][1] for c in GOAL)          # envs_per_task < rollouts_per_meta_task
    assert any(len(c[0][3]) == 3 for c in GOAL) and any(c[0][1] > 128 for c in GOAL) and any(c[0][1] == 1 for c in GOAL)
    assert any(c[0][2] == 1 for c in GOAL) and any(c[9] for c in GOAL)
    assert {c[0] for c in FIXED} == {'corner', 'momentum'}


@pytest.mark.parametrize('dims,scale,noise,step,seed,clip_infos,wanted,data_seed,rollouts,origin', GOAL,
                         ids=['-'.join(str(v) for v in c[:4]).replace(' ', '') for c in GOAL])
def test_gpu_case_is_sound(dims, scale, noise, step, seed, clip_infos, wanted, data_seed, rollouts, origin):
    pc.goal_case_is_sound(*dims, normalization_scale=scale, noise=noise, step=step, seed=seed, clip_infos=clip_infos, wanted=wanted,
                          data_seed=data_seed, rollouts=rollouts, origin=origin)


def test_sampler_accepts_the_classes_and_refuses_others():
    from promp_amd.envs import point_env
    from promp_amd.envs.normalized_env import normalize
    from promp_amd.samplers import device_point_sampler as dps
    for env, kind in ((point_env.MetaPointEnv(), 'origin'), (normalize(point_env.MetaPointEnvV2()), 'goal')):
        bare, opts = dps._point_env_options(env)
        assert dps._point_env_kind(bare) == kind and opts['max_step'] == 0.1 and opts['done_radius'] == 0.01
        assert opts['normalization_scale'] == (10.0 if kind == 'goal' else 0.0) and 'reward_type' not in opts
    with pytest.raises(AssertionError):
        dps._point_env_options(copy.copy(object()))
