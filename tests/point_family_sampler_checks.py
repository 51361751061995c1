"""DevicePointEnvSampler and the Trainer on MetaPointEnvWalls and MetaPointEnvMomentum, shared by test_emu_point_family_sampler.py
(emulator) and test_gpu_point_family_sampler.py (MI355X); modelled on run_device_rollout_scenario and run_trainer_scenario of
tests/test_plugin_api.py.  The caller has bound the library (promp_amd._lib.set_library_for_testing)."""
import numpy as np

from oracle import policy as op
from tests import point_family_checks as fc
from tests.rollout_checks import ATOL


def make_env(kind):
    from promp_amd.envs.normalized_env import normalize
    from promp_amd.envs.point_env import MetaPointEnvMomentum, MetaPointEnvWalls
    return normalize(MetaPointEnvWalls(reward_type='dense')) if kind == 'walls' else MetaPointEnvMomentum(reward_type='sparse')


def run_sampler_scenario(kind, M=3, B=4, T=15, hidden=(32, 32)):
    """host noise: the returned path dicts equal the NumPy class stepped on the RETURNED actions from the same start states
    (observations and rewards at ATOL); agent_infos carry the slab's means and log_std"""
    from promp_amd.policies.meta_gaussian_mlp_policy import MetaGaussianMLPPolicy
    from promp_amd.samplers.device_point_sampler import DevicePointEnvSampler
    np.random.seed(23)
    env = make_env(kind)
    O = fc.STATE_DIM[kind]
    policy = MetaGaussianMLPPolicy(name='p', obs_dim=O, action_dim=2, meta_batch_size=M, hidden_sizes=hidden)
    sampler = DevicePointEnvSampler(env=env, policy=policy, rollouts_per_meta_task=B, meta_batch_size=M, max_path_length=T)
    assert sampler.kind == kind and sampler.obs_dim == O
    state = np.random.get_state()
    sampler.update_tasks()
    np.random.set_state(state)
    tasks = env.sample_tasks(M)                                  # the same draws
    assert sampler.goals.shape == (M, 6 if kind == 'walls' else 2)
    spec = op.PolicySpec(O, 2, hidden)
    theta = spec.from_ordered_dict(policy.get_param_values())
    theta[-2:] = np.log(12.0)             # wide exploration: actions beyond the box, points that reach the walls
    policy.set_params(spec.to_ordered_dict(theta))
    policy.switch_to_pre_update()
    state = np.random.get_state()
    paths = sampler.obtain_samples()
    np.random.set_state(state)                                   # replay the sampler's draws
    start = np.random.uniform(-0.2, 0.2, size=(M, B, 2))
    if kind == 'momentum':
        start = np.concatenate((start, np.random.uniform(-0.1, 0.1, size=(M, B, 2))), axis=2)
    assert list(paths.keys()) == list(range(M)) and all(len(paths[i]) == B for i in range(M))
    bare = env.wrapped_env if kind == 'walls' else env
    scale = 10.0 if kind == 'walls' else 0.0
    events, margin = set(), np.inf
    for i in range(M):
        env.set_task(tasks[i])
        params = np.concatenate([tasks[i][k] for k in ('goal', 'gap_1', 'gap_2')]) if kind == 'walls' else tasks[i]
        np.testing.assert_array_equal(sampler.goals[i], params)
        for b in range(B):
            p = paths[i][b]
            assert p['observations'].shape == (T, O) and p['actions'].shape == (T, 2) and p['rewards'].shape == (T,)
            env.reset()
            fc.set_env_state(kind, bare, start[i, b])
            s = start[i, b]
            for t in range(T):
                np.testing.assert_allclose(p['observations'][t], s.astype(np.float32), rtol=0, atol=ATOL)
                _, _, info = fc.env_step(kind, s[None, :], p['actions'][t][None, :].astype(np.float64), params, reward_type=bare.reward_type,
                                         normalization_scale=scale, max_step=fc.MAX_STEP[kind], sparse_radius=2.0)
                events.add(int(info['event'][0]))
                margin = min(margin, float(info['margin'][0]))
                s, r, done, _ = env.step(p['actions'][t].astype(np.float64))
                assert done is False
                np.testing.assert_allclose(p['rewards'][t], r, rtol=0, atol=ATOL)
            mean = op.forward(spec, theta, p['observations'].astype(np.float64), False)[0]
            np.testing.assert_allclose(p['agent_infos']['mean'], mean, rtol=0, atol=ATOL)
            rows = slice((i * B + b) * T, (i * B + b + 1) * T)
            np.testing.assert_array_equal(p['agent_infos']['mean'], paths.flat['old_mean'][rows])
            np.testing.assert_array_equal(p['agent_infos']['log_std'], np.tile(paths.flat['old_log_std'][i], (T, 1)))
            np.testing.assert_allclose(p['agent_infos']['log_std'][0], np.log(12.0), rtol=0, atol=1e-6)
    assert margin >= fc.MARGIN                       # the NumPy class and the device saw the same side of every comparison
    if kind == 'walls':
        assert 1 in events                           # the inner wall threw a point back
    acts = np.concatenate([p['actions'] for i in range(M) for p in paths[i]])
    assert (np.abs(acts) > (scale if scale > 0 else fc.MAX_STEP[kind])).any()
    assert sampler.total_timesteps_sampled == M * B * T and paths.device_ref is not None


def run_trainer_scenario(kind, n_itr=3, M=2, P=3, T=12):
    """ProMP with device rollouts: every logged value is finite, the parameters move"""
    from promp_amd.baselines.linear_baseline import LinearFeatureBaseline
    from promp_amd.meta_algos.pro_mp import ProMP
    from promp_amd.meta_trainer import Trainer
    from promp_amd.policies.meta_gaussian_mlp_policy import MetaGaussianMLPPolicy
    from promp_amd.samplers.device_point_sampler import DevicePointEnvSampler
    from promp_amd.samplers.meta_sample_processor import MetaSampleProcessor
    from promp_amd.utils import logger
    logger.configure(dir=None, snapshot_mode='last', quiet=True)
    np.random.seed(1)
    env = make_env(kind)
    policy = MetaGaussianMLPPolicy(name='meta-policy', obs_dim=fc.STATE_DIM[kind], action_dim=2, meta_batch_size=M, hidden_sizes=(32, 32))
    sampler = DevicePointEnvSampler(env=env, policy=policy, rollouts_per_meta_task=P, meta_batch_size=M, max_path_length=T)
    proc = MetaSampleProcessor(baseline=LinearFeatureBaseline(), discount=0.99, gae_lambda=1, normalize_adv=True)
    algo = ProMP(policy=policy, inner_lr=0.1, meta_batch_size=M, num_inner_grad_steps=1, learning_rate=1e-3, num_ppo_steps=2,
                 clip_eps=0.3, init_inner_kl_penalty=5e-4, adaptive_inner_kl_penalty=False)
    trainer = Trainer(algo=algo, policy=policy, env=env, sampler=sampler, sample_processor=proc, n_itr=n_itr, num_inner_grad_steps=1)
    before = policy.get_param_values()
    seen, rounds = {}, []
    orig = logger.dumpkvs

    def grab():
        seen.update(logger.getkvs())
        rounds.append(dict(logger.getkvs()))
        return orig()
    logger.dumpkvs = grab
    try:
        trainer.train()
    finally:
        logger.dumpkvs = orig
    assert len(rounds) == n_itr and seen['n_timesteps'] == n_itr * 2 * M * P * T
    for kvs in rounds:
        for k in ('Step_0-AverageReturn', 'Step_1-AverageReturn', 'Step_1-AverageDiscountedReturn', 'Step_0-StdReturn', 'LossBefore',
                  'LossAfter', 'KLInner'):
            assert k in kvs, k
        for k, v in kvs.items():
            if isinstance(v, (int, float, np.floating, np.integer)):
                assert np.isfinite(v), (k, v)
    after = policy.get_param_values()
    assert any(np.any(before[k] != after[k]) for k in before) and all(np.all(np.isfinite(v)) for v in after.values())
