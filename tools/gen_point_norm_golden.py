"""Write tests/golden/point_env_norm_{corner,momentum,goal}.npz: what the REFERENCE's normalize wrapper returns and keeps when its
running observation / reward normalisation is on (envs/normalized_env.py:73-123: normalize(env, normalize_obs=..., normalize_reward=...,
obs_alpha=..., reward_alpha=...)), around MetaPointEnvCorner, MetaPointEnvMomentum and the MetaPointEnv of point_env_2d_v2.py.  They pin
the NumPy replay tests/point_norm_checks.py:norm_update / replay_calls, promp_amd.envs.normalized_env.NormalizedEnv and through them
the device (promp_collect_point_family_norm).

    python tools/gen_point_norm_golden.py /path/to/the/reference/checkout

The reference is imported the way tools/gen_point_family_golden.py does.  Needs nothing but NumPy.

Each fixture holds data only.  One sequence of wrapper calls is driven through four wrappers, one per flag combination
flags [4][2] = (normalize_obs, normalize_reward), obs_alpha 0.1 and reward_alpha 0.2 (with the default 0.001 a wrong update order
hides below float32):
  is_reset [n]            call c is reset() (True) or step(actions[c]) (False); call 0 is a reset, resets follow steps directly, two
                          resets follow one another once, and the sequence ends with a reset behind a step
  reset_states [n][O]     the raw state the bare environment's reset() is made to produce at call c (zeros at steps)
  actions [n][2]          policy-scale actions (zeros at resets), some beyond the wrapper's box
  observations [4][n][O]  what the wrapper returned; rewards [4][n], dones [4][n] (0 at resets)
  obs_mean, obs_var [4][n][O], reward_mean, reward_var [4][n]   the wrapper's _obs_mean, _obs_var, _reward_mean, _reward_var AFTER call c
  task [2], normalization_scale, obs_alpha, reward_alpha, action_high"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_point_family_golden import GOLDEN, import_reference, quiet  # noqa: E402

FLAGS = [(False, False), (True, False), (False, True), (True, True)]
OBS_ALPHA, REWARD_ALPHA = 0.1, 0.2
# calls: R reset, S step
SEQUENCE = 'RSSSRSRRSSSSSRSSRSSSSSSSRSR'


def gen(name, make_bare, normalize, seed):
    rng = np.random.RandomState(seed)
    O = 4 if name == 'momentum' else 2
    n = len(SEQUENCE)
    is_reset = np.array([c == 'R' for c in SEQUENCE])
    np.random.seed(seed)
    task = np.asarray(quiet(make_bare).sample_tasks(1)[0], np.float64)
    spread = 0.05 if name == 'goal' else 0.2
    reset_states = np.where(is_reset[:, None], rng.uniform(-spread, spread, size=(n, O)), 0.0)
    if name == 'momentum':
        reset_states[:, 2:] *= 0.5
    actions = np.where(is_reset[:, None], 0.0, rng.randn(n, 2) * 6.0)
    obs, rew, dones = np.zeros((4, n, O)), np.zeros((4, n)), np.zeros((4, n), bool)
    om, ov, rm, rv = np.zeros((4, n, O)), np.zeros((4, n, O)), np.zeros((4, n)), np.zeros((4, n))
    for f, (n_obs, n_rew) in enumerate(FLAGS):
        bare = quiet(make_bare)
        env = normalize(bare, normalize_obs=n_obs, normalize_reward=n_rew, obs_alpha=OBS_ALPHA, reward_alpha=REWARD_ALPHA)
        env.set_task(task)
        call = [0]

        def reset():                         # the bare class's reset() with the drawn state replaced by the recorded one
            s = reset_states[call[0]]
            bare._state = s[:2].copy()
            if name == 'momentum':
                bare._velocity = s[2:].copy()
                return np.hstack((bare._state, bare._velocity))
            return np.copy(bare._state)
        bare.reset = reset
        for c in range(n):
            call[0] = c
            if is_reset[c]:
                obs[f, c] = env.reset()
            else:
                o, r, d, info = env.step(actions[c])
                obs[f, c], rew[f, c], dones[f, c] = o, r, bool(d)
            om[f, c], ov[f, c], rm[f, c], rv[f, c] = env._obs_mean, env._obs_var, env._reward_mean, env._reward_var
        scale, high = float(env._normalization_scale), np.asarray(bare.action_space.high, np.float64)
    assert (np.abs(actions) > scale).any() and is_reset[-1] and not is_reset[-2]
    assert np.any(om[1] != 0) and not np.any(om[0] != 0) and np.all(ov[0] == 1) and np.any(rv[2] != 1) and np.all(rv[1] == 1)
    np.savez(os.path.join(GOLDEN, 'point_env_norm_%s.npz' % name), seed=seed, task=task, flags=np.array(FLAGS), is_reset=is_reset,
             reset_states=reset_states, actions=actions, observations=obs, rewards=rew, dones=dones, obs_mean=om, obs_var=ov,
             reward_mean=rm, reward_var=rv, normalization_scale=scale, obs_alpha=OBS_ALPHA, reward_alpha=REWARD_ALPHA, action_high=high)
    print('wrote point_env_norm_%s.npz  %d calls, %d resets, %d dones' % (name, n, int(is_reset.sum()), int(dones[0].sum())))


if __name__ == '__main__':
    _, Momentum, normalize = import_reference(sys.argv[1])
    from meta_policy_search.envs.point_envs.point_env_2d_corner import MetaPointEnvCorner as Corner
    from meta_policy_search.envs.point_envs.point_env_2d_v2 import MetaPointEnv as Goal
    gen('corner', lambda: Corner(reward_type='dense'), normalize, 61)
    gen('momentum', lambda: Momentum(reward_type='dense_squared'), normalize, 62)
    gen('goal', Goal, normalize, 63)
