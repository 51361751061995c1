"""2-D point-mass meta-environments: MetaPointEnvCorner, the environment of BASELINE config 1
(run_scripts/pro-mp_run_point_mass.py trains on normalize(MetaPointEnvCorner())), its two fixed-horizon siblings with corner goals,
MetaPointEnvWalls and MetaPointEnvMomentum, and the two whose episodes end early, MetaPointEnv and MetaPointEnvV2 (described at
the classes).

Behaviour (reference: meta_policy_search/envs/point_envs/point_env_2d_corner.py:13-93, MetaEnv interface envs/base.py:6-49):
  * a task is a goal, one of the corners (-2,-2), (2,-2), (-2,2), (2,2), drawn uniformly;
  * reset: state ~ U(-0.2, 0.2)^2; step: state += clip(action, -0.2, 0.2); an episode never ends by itself;
  * reward_type 'dense': -|s' - goal|;  'dense_squared': -|s' - goal|^2;
    'sparse' (the default): nothing while the point is within L1 distance `sparse_reward_radius` of the origin, afterwards the
    progress |s - goal| - |s' - goal| if the goal is the corner nearest to s', else 0.
The device runs the same arithmetic in k_point_rollout (samplers/device_point_sampler.py); the trajectories of the reference
class are the golden vectors tests/golden/point_env_*.npz.
"""
import numpy as np

from .base import MetaEnv


class ActionBox(object):
    """just the attributes the normalize wrapper and the run scripts read from a gym.spaces.Box"""

    def __init__(self, low, high, shape):
        self.low = np.full(shape, low, dtype=np.float64)
        self.high = np.full(shape, high, dtype=np.float64)
        self.shape = tuple(shape)


class MetaPointEnvCorner(MetaEnv):
    CORNERS = np.array([[-2.0, -2.0], [2.0, -2.0], [-2.0, 2.0], [2.0, 2.0]])

    def __init__(self, reward_type='sparse', sparse_reward_radius=0.5):
        assert reward_type in ('dense', 'dense_squared', 'sparse')
        self.reward_type = reward_type
        self.sparse_reward_radius = sparse_reward_radius
        self.corners = [c.copy() for c in self.CORNERS]
        self.observation_space = ActionBox(-np.inf, np.inf, (2,))
        self.action_space = ActionBox(-0.2, 0.2, (2,))
        self.goal = self.corners[3]
        self._state = np.zeros(2)

    # ---- MetaEnv ----
    def sample_tasks(self, n_tasks):
        return [self.corners[k] for k in np.random.choice(len(self.corners), size=n_tasks)]

    def set_task(self, task):
        self.goal = np.asarray(task, dtype=np.float64)

    def get_task(self):
        return self.goal

    def log_diagnostics(self, *args, **kwargs):
        pass

    # ---- dynamics ----
    def reset(self):
        self._state = np.random.uniform(-0.2, 0.2, size=(2,))
        return self._state.copy()

    def step(self, action):
        before = self._state
        self._state = before + np.clip(action, self.action_space.low, self.action_space.high)
        return self._state.copy(), self.reward(before, action, self._state), False, {}

    @staticmethod
    def _distance(a, b):
        d = np.asarray(a, dtype=np.float64) - b
        return np.sqrt(np.sum(d * d))          # (sum of squares, then root: the rounding of a row-wise 2-norm)

    def reward(self, obs, act, obs_next):
        to_goal = self._distance(obs_next, self.goal)
        if self.reward_type == 'dense':
            return -to_goal
        if self.reward_type == 'dense_squared':
            return -to_goal ** 2
        if np.sum(np.abs(obs_next)) < self.sparse_reward_radius:
            return 0
        if to_goal == min(self._distance(obs_next, corner) for corner in self.corners):
            return self._distance(obs, self.goal) - to_goal
        return 0


def _norm(v):
    v = np.asarray(v, dtype=np.float64)
    return np.sqrt(np.sum(v * v))              # (sum of squares, then root, as _distance)


class MetaPointEnvWalls(MetaEnv):
    """The point mass behind two circular walls (reference: envs/point_envs/point_env_2d_walls.py:7-107).

      * a task is dict(goal, gap_1, gap_2): a corner drawn uniformly, and one point on the circle of radius 1 and one on the circle
        of radius 2, each a normalised standard-normal draw; a wall is open within distance 1 of its gap;
      * reset: state ~ U(-0.2, 0.2)^2; step: s' = s + clip(action, -0.2, 0.2), the reward is taken on this s', and then
          if |s| < 1 and |s'| > 1:       s' <- s' / (|s'| + 1e-6)      unless |s' - gap_1| <= 1   (thrown back onto the inner wall)
          elif |s| < 2 and |s'| > 2:     s' <- s' / (0.5 |s'| + 1e-6)  unless |s' - gap_2| <= 1   (the outer wall)
        an episode never ends by itself;
      * reward_type 'dense' (the default): -|s' - goal|; 'dense_squared': -|s' - goal|^2; 'sparse': the progress
        |s - goal| - |s' - goal| while |s' - goal| < sparse_reward_radius.  Outside the radius the reference returns None, which its
        own normalize wrapper raises on and no sampler can sum: here that reward is 0.0.
    The reference's assertions on the projected state are not reproduced.  The device runs the same arithmetic
    (promp_rollout_point_family, kind walls); the trajectories of the reference class are tests/golden/point_env_walls_*.npz."""
    CORNERS = MetaPointEnvCorner.CORNERS

    def __init__(self, reward_type='dense', sparse_reward_radius=2):
        assert reward_type in ('dense', 'dense_squared', 'sparse')
        self.reward_type = reward_type
        self.sparse_reward_radius = sparse_reward_radius
        self.corners = [c.copy() for c in self.CORNERS]
        self.observation_space = ActionBox(-np.inf, np.inf, (2,))
        self.action_space = ActionBox(-0.2, 0.2, (2,))
        self.goal, self.gap_1, self.gap_2 = self.corners[3], np.array([1.0, 0.0]), np.array([2.0, 0.0])
        self._state = np.zeros(2)

    # ---- MetaEnv ----
    def sample_tasks(self, n_tasks):
        goals = [self.corners[k] for k in np.random.choice(len(self.corners), size=n_tasks)]
        gaps_1 = np.random.normal(size=(n_tasks, 2))
        gaps_1 /= np.linalg.norm(gaps_1, axis=1)[:, None]
        gaps_2 = np.random.normal(size=(n_tasks, 2))
        gaps_2 /= (np.linalg.norm(gaps_2, axis=1) / 2)[:, None]
        return [dict(goal=g, gap_1=g1, gap_2=g2) for g, g1, g2 in zip(goals, gaps_1, gaps_2)]

    def set_task(self, task):
        self.goal = np.asarray(task['goal'], dtype=np.float64)
        self.gap_1 = np.asarray(task['gap_1'], dtype=np.float64)
        self.gap_2 = np.asarray(task['gap_2'], dtype=np.float64)

    def get_task(self):
        return dict(goal=self.goal, gap_1=self.gap_1, gap_2=self.gap_2)

    def log_diagnostics(self, *args, **kwargs):
        pass

    # ---- dynamics ----
    def reset(self):
        self._state = np.random.uniform(-0.2, 0.2, size=(2,))
        return self._state.copy()

    def step(self, action):
        before = self._state
        after = before + np.clip(action, self.action_space.low, self.action_space.high)
        reward = self.reward(before, action, after)
        if _norm(before) < 1 and _norm(after) > 1:
            if _norm(after - self.gap_1) > 1:
                after = after / (_norm(after) + 1e-6)
        elif _norm(before) < 2 and _norm(after) > 2:
            if _norm(after - self.gap_2) > 1:
                after = after / (_norm(after) * 0.5 + 1e-6)
        self._state = after
        return after.copy(), reward, False, {}

    def reward(self, obs, act, obs_next):
        to_goal = _norm(obs_next - self.goal)
        if self.reward_type == 'dense':
            return -to_goal
        if self.reward_type == 'dense_squared':
            return -to_goal ** 2
        if to_goal < self.sparse_reward_radius:
            return _norm(obs - self.goal) - to_goal
        return 0.0


class MetaPointEnvMomentum(MetaEnv):
    """The point mass steered by accelerations (reference: envs/point_envs/point_env_2d_momentum.py:7-88).

      * a task is a goal, one of the four corners, drawn uniformly;
      * reset: position ~ U(-0.2, 0.2)^2, velocity ~ U(-0.1, 0.1)^2; step: v <- v + clip(action, -0.1, 0.1), s' = s + v;
        the observation is (s'_0, s'_1, v_0, v_1); an episode never ends by itself;
      * reward_type 'dense': -|s' - goal|; 'dense_squared': -|s' - goal|^2; 'sparse' (the default):
        max(sparse_reward_radius - |s' - goal|, 0).
    The device runs the same arithmetic (promp_rollout_point_family, kind momentum); the trajectories of the reference class are
    tests/golden/point_env_momentum_*.npz."""
    CORNERS = MetaPointEnvCorner.CORNERS

    def __init__(self, reward_type='sparse', sparse_reward_radius=2):
        assert reward_type in ('dense', 'dense_squared', 'sparse')
        self.reward_type = reward_type
        self.sparse_reward_radius = sparse_reward_radius
        self.corners = [c.copy() for c in self.CORNERS]
        self.observation_space = ActionBox(-np.inf, np.inf, (4,))
        self.action_space = ActionBox(-0.1, 0.1, (2,))
        self.goal = self.corners[3]
        self._state, self._velocity = np.zeros(2), np.zeros(2)

    # ---- MetaEnv ----
    def sample_tasks(self, n_tasks):
        return [self.corners[k] for k in np.random.choice(len(self.corners), size=n_tasks)]

    def set_task(self, task):
        self.goal = np.asarray(task, dtype=np.float64)

    def get_task(self):
        return self.goal

    def log_diagnostics(self, *args, **kwargs):
        pass

    # ---- dynamics ----
    def reset(self):
        self._state = np.random.uniform(-0.2, 0.2, size=(2,))
        self._velocity = np.random.uniform(-0.1, 0.1, size=(2,))
        return np.hstack((self._state, self._velocity))

    def step(self, action):
        before = self._state
        self._velocity = self._velocity + np.clip(action, self.action_space.low, self.action_space.high)
        self._state = before + self._velocity
        return np.hstack((self._state, self._velocity)), self.reward(before, action, self._state), False, {}

    def reward(self, obs, act, obs_next):
        to_goal = _norm(np.asarray(obs_next, dtype=np.float64)[:2] - self.goal)
        if self.reward_type == 'dense':
            return -to_goal
        if self.reward_type == 'dense_squared':
            return -to_goal ** 2
        return max(self.sparse_reward_radius - to_goal, 0.0)


class MetaPointEnv(MetaEnv):
    """The point mass that has to reach the origin, and whose episode ENDS there (reference: envs/point_envs/point_env_2d.py:7-71;
    corner_goals_point_env_2d.py is the same class).

      * a task is {}: every task is the same environment;
      * reset: state ~ U(-2, 2)^2; step: s' = s + clip(action, -0.1, 0.1); reward -|s'|;
      * done: |s'_0| < 0.01 and |s'_1| < 0.01 (a box around the origin, not a disc).
    There is no reward_type.  The device runs the same arithmetic (promp_collect_point_family, kind goal with the goal (0, 0):
    (0 - x)^2 and x^2 are the same bits); the trajectories of the reference class are tests/golden/point_env_origin.npz."""
    DONE_RADIUS = 0.01

    def __init__(self):
        self.observation_space = ActionBox(-np.inf, np.inf, (2,))
        self.action_space = ActionBox(-0.1, 0.1, (2,))
        self._state = np.zeros(2)

    # ---- MetaEnv ----
    def sample_tasks(self, n_tasks):
        return [{}] * n_tasks

    def set_task(self, task):
        pass

    def get_task(self):
        return {}

    def log_diagnostics(self, *args, **kwargs):
        pass

    # ---- dynamics ----
    def reset(self):
        self._state = np.random.uniform(-2, 2, size=(2,))
        return self._state.copy()

    def step(self, action):
        before = self._state
        self._state = before + np.clip(action, self.action_space.low, self.action_space.high)
        return self._state.copy(), self.reward(before, action, self._state), self.done(self._state), {}

    def done(self, obs):
        return bool(abs(obs[0]) < self.DONE_RADIUS and abs(obs[1]) < self.DONE_RADIUS)

    def reward(self, obs, act, obs_next):
        return -_norm(obs_next)


class MetaPointEnvV2(MetaPointEnv):
    """The point mass that starts at the origin and is rewarded for reaching a goal (reference: envs/point_envs/point_env_2d_v2.py:7-75).

      * a task is a goal ~ U(-2, 2)^2;
      * reset: state = (0, 0); step: s' = s + clip(action, -0.1, 0.1); reward -|goal - s'|;
      * done: |s'_0| < 0.01 and |s'_1| < 0.01 -- the box around the ORIGIN, not around the goal, exactly as the reference has it: an
        episode ends when the point is back where it started (so every first step smaller than 0.01 ends one).  The quirk is kept.
    The reference's get_task reads self.task, an attribute it never sets; here get_task returns the goal.  The device runs the same
    arithmetic (promp_collect_point_family, kind goal); the reference's trajectories are tests/golden/point_env_goal.npz."""

    def __init__(self):
        super(MetaPointEnvV2, self).__init__()
        self.goal = np.random.uniform(-2, 2, size=(2,))

    def sample_tasks(self, n_tasks):
        return np.random.uniform(-2, 2, size=(n_tasks, 2))

    def set_task(self, task):
        self.goal = np.asarray(task, dtype=np.float64)

    def get_task(self):
        return self.goal

    def reset(self):
        self._state = np.zeros(2)
        return self._state.copy()

    def reward(self, obs, act, obs_next):
        return -_norm(self.goal - obs_next)


POINT_ENVS = dict(corner=MetaPointEnvCorner, walls=MetaPointEnvWalls, momentum=MetaPointEnvMomentum, origin=MetaPointEnv,
                  goal=MetaPointEnvV2)


def make_point_env(name='corner', reward_type=None):
    """name: 'corner' | 'walls' | 'momentum' | 'origin' | 'goal' or the class's name; reward_type None: the class's default (the
    two terminating classes, origin and goal, have none)"""
    classes = dict(POINT_ENVS, **{cls.__name__: cls for cls in POINT_ENVS.values()})
    assert name in classes, 'unknown point-mass environment %r (one of %s)' % (name, ', '.join(sorted(POINT_ENVS)))
    if issubclass(classes[name], MetaPointEnv):
        assert reward_type is None, 'MetaPointEnv and MetaPointEnvV2 have no reward_type (asked for %r)' % (reward_type,)
    return classes[name]() if reward_type is None else classes[name](reward_type=reward_type)
