"""2-D point-mass meta-environments with corner goals: MetaPointEnvCorner, the environment of BASELINE config 1
(run_scripts/pro-mp_run_point_mass.py trains on normalize(MetaPointEnvCorner())), and its two fixed-horizon siblings
MetaPointEnvWalls and MetaPointEnvMomentum (described at the classes).

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


MetaPointEnv = MetaPointEnvCorner      # (the name earlier revisions of this package used)


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


POINT_ENVS = dict(corner=MetaPointEnvCorner, walls=MetaPointEnvWalls, momentum=MetaPointEnvMomentum)


def make_point_env(name='corner', reward_type=None):
    """name: 'corner' | 'walls' | 'momentum' or the class's name; reward_type None: the class's default"""
    classes = dict(POINT_ENVS, **{cls.__name__: cls for cls in POINT_ENVS.values()})
    assert name in classes, 'unknown point-mass environment %r (one of %s)' % (name, ', '.join(sorted(POINT_ENVS)))
    return classes[name]() if reward_type is None else classes[name](reward_type=reward_type)
