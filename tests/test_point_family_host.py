"""MetaPointEnvWalls and MetaPointEnvMomentum on the CPU: the reference classes' trajectories (tests/golden/point_env_walls_*.npz,
point_env_momentum_*.npz) pin the float64 restatement tests.point_family_checks.env_step, which the device tests compare with, and
the package's own NumPy classes; sample_tasks draws the reference's tasks from a seeded np.random."""
import numpy as np
import pytest

from promp_amd.envs import point_env
from tests import point_family_checks as fc

CASES = [(k, r) for k in fc.KINDS for r in fc.REWARDS]


@pytest.fixture(scope='module', params=CASES, ids=['%s-%s' % c for c in CASES])
def fixture(request):
    kind, reward_type = request.param
    g, tasks, env = fc.load_fixture(kind, reward_type)
    return kind, reward_type, g, tasks, env


def test_fixtures_hold_what_they_are_for(fixture):
    kind, reward_type, g, tasks, env = fixture
    assert env['max_step'] == fc.MAX_STEP[kind] and env['sparse_radius'] == 2.0
    box = env['normalization_scale'] if env['normalization_scale'] > 0 else env['max_step']
    assert (np.abs(g['actions']) > box).any()
    if kind == 'walls':
        assert set(np.unique(g['events'])) == {0, 1, 2, 3, 4}
        assert (env['normalization_scale'] == 0) == (reward_type == 'sparse')
        assert g['reward_is_none'].any() == (reward_type == 'sparse')
    if reward_type == 'sparse':
        assert 0 < np.count_nonzero(g['rewards']) < g['rewards'].size
    if kind == 'momentum' and env['normalization_scale'] > 0:
        assert (np.abs(g['actions']) > 10).any()


def test_restatement_matches_the_reference_trajectories(fixture):
    kind, reward_type, g, tasks, env = fixture
    for b in range(len(tasks)):
        state = g['start'][b][None, :]
        for t in range(g['actions'].shape[1]):
            state, rew, info = fc.env_step(kind, state, g['actions'][b, t][None, :], tasks[b], **env)
            np.testing.assert_allclose(state[0], g['next_observations'][b, t], rtol=0, atol=1e-12)
            np.testing.assert_allclose(rew[0], g['rewards'][b, t], rtol=0, atol=1e-12)
            if kind == 'walls':
                assert info['event'][0] == g['events'][b, t], (b, t)
                assert (rew[0] == 0.0) or not g['reward_is_none'][b, t]


def test_restatement_is_batched(fixture):
    """all the fixture's environments of one task index at once give what one at a time gives"""
    kind, reward_type, g, tasks, env = fixture
    state = np.repeat(g['start'][:1], 3, axis=0) + np.array([0.0, 0.01, -0.02])[:, None]
    nxt, rew, info = fc.env_step(kind, state, np.repeat(g['actions'][0, :1], 3, axis=0), tasks[0], **env)
    for j in range(3):
        one, r1, i1 = fc.env_step(kind, state[j:j + 1], g['actions'][0, :1], tasks[0], **env)
        assert np.array_equal(one[0], nxt[j]) and r1[0] == rew[j] and i1['event'][0] == info['event'][j]


def test_numpy_classes_match_the_reference_trajectories(fixture):
    kind, reward_type, g, tasks, env = fixture
    wrapped, bare = fc.make_env(kind, reward_type, env['normalization_scale'])
    assert bare.sparse_reward_radius == 2 and bare.observation_space.shape == (fc.STATE_DIM[kind],)
    np.testing.assert_array_equal(bare.action_space.high, g['action_high'])
    np.testing.assert_array_equal(bare.action_space.low, g['action_low'])
    for b in range(len(tasks)):
        wrapped.set_task(fc.task_of(kind, tasks[b]))
        assert wrapped.reset().shape == (fc.STATE_DIM[kind],)
        fc.set_env_state(kind, bare, g['start'][b])
        for t in range(g['actions'].shape[1]):
            obs, rew, done, info = wrapped.step(g['actions'][b, t])
            assert done is False and info == {}
            np.testing.assert_allclose(obs, g['next_observations'][b, t], rtol=0, atol=1e-12)
            np.testing.assert_allclose(rew, g['rewards'][b, t], rtol=0, atol=1e-12)


def test_sample_tasks_draws_the_reference_tasks(fixture):
    kind, reward_type, g, tasks, env = fixture
    wrapped, bare = fc.make_env(kind, reward_type, env['normalization_scale'])
    np.random.seed(int(g['seed']))
    drawn = wrapped.sample_tasks(len(tasks))
    if kind == 'walls':
        assert all(sorted(d) == ['gap_1', 'gap_2', 'goal'] for d in drawn)
        drawn = [np.concatenate((d['goal'], d['gap_1'], d['gap_2'])) for d in drawn]
        np.testing.assert_allclose(np.linalg.norm(np.asarray(drawn)[:, 2:4], axis=1), 1.0, atol=1e-12)
        np.testing.assert_allclose(np.linalg.norm(np.asarray(drawn)[:, 4:6], axis=1), 2.0, atol=1e-12)
    assert np.array_equal(np.asarray(drawn, np.float64), tasks)


def test_defaults_and_reset():
    walls, mom = point_env.MetaPointEnvWalls(), point_env.MetaPointEnvMomentum()
    assert (walls.reward_type, walls.sparse_reward_radius) == ('dense', 2)
    assert (mom.reward_type, mom.sparse_reward_radius) == ('sparse', 2)
    np.random.seed(3)
    s = walls.reset()
    o = mom.reset()
    np.random.seed(3)
    assert np.array_equal(s, np.random.uniform(-0.2, 0.2, size=2))
    assert np.array_equal(o, np.hstack((np.random.uniform(-0.2, 0.2, size=2), np.random.uniform(-0.1, 0.1, size=2))))
    task = walls.sample_tasks(1)[0]
    walls.set_task(task)
    assert all(np.array_equal(walls.get_task()[k], task[k]) for k in task)
    with pytest.raises(AssertionError):
        point_env.MetaPointEnvWalls(reward_type='nothing')
