"""DevicePointEnvSampler(device_starts=True, device_noise=True), shared by test_emu_point_start_sampler.py (emulator, tiny) and
test_gpu_point_start_sampler.py (MI355X).  The caller of the sampler scenarios has bound the library
(promp_amd._lib.set_library_for_testing).

Per class (corner, walls, momentum, MetaPointEnv 'origin', MetaPointEnvV2 'goal'), without observation normalisation:
  * the first observation of every returned path is float32 of point_start_checks.start_rows -- the NumPy restatement of the draw --
    for the path's (path_start row, environment) under sampler.last_seed and the step slot (a fixed-horizon slab has row 0 only);
  * np.random's state after obtain_samples is that of a twin generator that drew exactly one randint(0, 2 ** 31 - 1), whose value is
    sampler.last_seed;
  * two consecutive sampling steps differ; MetaPointEnvV2 starts every path at exactly 0.
Under normalize_obs=True, normalize_reward=True the sampler's get_normalization_state() equals, bit for bit, the moments a context of
the test's own is left with by the TABLE entry point (promp_collect_point_family_norm) handed the restated table, the same policy,
tasks, seed and step slot.  check_feeds_the_stack is point_collect_checks.check_feeds_the_stack with the start states drawn on the
device: the resident slabs through process_samples, inner_adapt and optimize against the same slabs downloaded and uploaded again."""
import numpy as np

from oracle import policy as op
from promp_amd import _lib
from tests import point_collect_checks as pc, point_norm_checks as pn, point_start_checks as ps
from tests.rollout_checks import MIN_STD, SEED64

CLASSES = ('corner', 'walls', 'momentum', 'origin', 'goal')
BOX = dict(corner=ps.CORNER_BOX, walls=ps.CORNER_BOX, momentum=ps.MOMENTUM_BOX, origin=ps.ORIGIN_BOX, goal=dict(lo=[0.0, 0.0], hi=[0.0, 0.0]))


def make_sampler(name, M, B, R, T, hidden, **wrapper):
    from promp_amd.envs import point_env
    from promp_amd.envs.normalized_env import normalize
    from promp_amd.policies.meta_gaussian_mlp_policy import MetaGaussianMLPPolicy
    from promp_amd.samplers.device_point_sampler import DevicePointEnvSampler
    bare = dict(corner=point_env.MetaPointEnvCorner, walls=point_env.MetaPointEnvWalls, momentum=point_env.MetaPointEnvMomentum,
                origin=point_env.MetaPointEnv, goal=point_env.MetaPointEnvV2)[name]()
    env = normalize(bare, **wrapper)
    O = 4 if name == 'momentum' else 2
    policy = MetaGaussianMLPPolicy(name='p', obs_dim=O, action_dim=2, meta_batch_size=M, hidden_sizes=hidden)
    sampler = DevicePointEnvSampler(env=env, policy=policy, rollouts_per_meta_task=R, meta_batch_size=M, max_path_length=T,
                                    envs_per_task=B, device_noise=True, device_starts=True)
    spec = op.PolicySpec(O, 2, hidden)
    theta = spec.from_ordered_dict(policy.get_param_values())
    theta[-2:] = np.log(0.8)
    policy.set_params(spec.to_ordered_dict(theta))
    policy.switch_to_pre_update()
    return sampler, policy, theta, O


def sample_once(sampler):
    """one obtain_samples -> (paths, first observations [n_paths, O], their start-table rows, the step slot); asserts the one draw"""
    before = np.random.get_state()
    paths = sampler.obtain_samples()
    after = np.random.get_state()
    np.random.set_state(before)                               # the twin: exactly one randint
    assert int(np.random.randint(0, 2 ** 31 - 1)) == sampler.last_seed
    twin = np.random.get_state()
    assert twin[0] == after[0] and np.array_equal(twin[1], after[1]) and twin[2:] == after[2:], 'the sampler drew more than one randint'
    np.random.set_state(after)
    fl = paths.flat
    n_envs = sampler.meta_batch_size * sampler.envs_per_task
    n_paths = len(fl['path_row_offsets']) - 1
    p_env = fl.get('path_env', np.arange(n_paths, dtype=np.int32))
    p_start = fl.get('path_start', np.zeros(n_paths, np.int32))
    rows = p_start.astype(np.int64) * n_envs + p_env
    return paths, fl['obs'][fl['path_row_offsets'][:-1]], rows, paths.device_ref[2]


def run_sampler_scenario(name, M=3, B=3, R=4, T=10, hidden=(32, 32)):
    np.random.seed(37)
    sampler, policy, theta, O = make_sampler(name, M, B, R, T, hidden)
    assert sampler.kind == name and sampler.device_starts and sampler.last_seed is None
    lo, hi = BOX[name]['lo'], BOX[name]['hi']
    seen = []
    for call in range(2):
        sampler.update_tasks()
        paths, first, rows, slot = sample_once(sampler)
        want = ps.start_rows(sampler.last_seed, slot, rows, O, lo, hi).astype(np.float32)
        assert first.shape == want.shape and np.array_equal(first, want), (name, call, np.abs(first - want).max())
        assert list(paths.keys()) == list(range(M)) and sum(len(paths[i]) for i in range(M)) == len(rows)
        assert paths[0][0]['observations'].shape[1] == O and np.array_equal(paths[0][0]['observations'][0], first[0])
        if name == 'goal':
            assert not first.any()                            # MetaPointEnvV2: every path from exactly 0
            assert len(set(np.diff(paths.flat['path_row_offsets']))) > 1          # (episodes do end early: rows beyond 0 were drawn)
        else:
            assert len(np.unique(first)) == first.size        # no two coordinates alike: every reset() has its own block
        seen.append((sampler.last_seed, paths.flat['obs'].copy()))
    assert seen[0][0] != seen[1][0]
    n = min(len(seen[0][1]), len(seen[1][1]))
    assert np.any(seen[0][1][:n] != seen[1][1][:n]), 'two consecutive sampling steps returned the same observations'


def run_normalised_scenario(name, M=3, B=3, R=4, T=10, hidden=(32, 32), obs_alpha=0.1, reward_alpha=0.2):
    np.random.seed(41)
    sampler, policy, theta, O = make_sampler(name, M, B, R, T, hidden, normalize_obs=True, normalize_reward=True, obs_alpha=obs_alpha,
                                             reward_alpha=reward_alpha)
    B = sampler.envs_per_task
    N = M * B
    norm = dict(normalize_obs=True, normalize_reward=True, obs_alpha=obs_alpha, reward_alpha=reward_alpha)
    state = lambda: pn.join_moments(*[sampler.get_normalization_state()[k] for k in ('obs_mean', 'obs_var', 'reward_mean', 'reward_var')])
    terminating = name in ('origin', 'goal')
    S = pc.max_steps_of(M, B, T, M * R * T) if terminating else T
    total = M * R * T if terminating else N * T
    for call in range(2):
        sampler.update_tasks()
        before = state()
        paths, _, _, slot = sample_once(sampler)
        after = state()
        assert np.any(after != before)
        lo, hi = BOX[name]['lo'], BOX[name]['hi']
        table = ps.start_table(sampler.last_seed, slot, S + 1, N, O, lo, hi)
        K = policy.session.ctx.dims.num_inner_steps
        ctx = _lib.Context(M, O, 2, hidden, K, max_rows=S * N, max_paths=S * N)
        try:
            ctx.set_min_std(policy.session.min_std)
            ctx.set_theta(theta.astype(np.float32))
            ctx.switch_to_pre_update()
            ctx.set_point_norm(before)
            got = ctx.collect_point_family(slot, 'goal' if terminating else name, sampler.goals, table, None, total_samples=total,
                                           max_path_length=T, clip_infos=True, seed=sampler.last_seed, norm=norm, **sampler._env_opts)
            ref_after = ctx.get_point_norm(N, O)
            ref_obs = ctx.download_step(slot)['obs']
        finally:
            ctx.close()
        assert np.array_equal(got['path_row_offsets'], paths.flat['path_row_offsets'])
        assert np.array_equal(ref_obs, paths.flat['obs'])
        assert np.array_equal(after, ref_after), (name, call, np.abs(after - ref_after).max())


def check_feeds_the_stack(lib, M, B, T, hidden, seed=SEED64, data_seed=0):
    """collected goal slabs (steps 0 and 1, device noise AND device starts) through process_samples, inner_adapt and one ProMP
    optimize, against the same paths uploaded from the host into a second context: rtol 1e-6, atol 1e-7"""
    c = pc.goal_case(M, B, T, hidden, 10, 'device', 0, seed, data_seed)
    alpha, eta = 0.1, np.array([5e-4], np.float32)
    opts = dict(discount=0.99, gae_lambda=1.0, normalize_adv=True)
    theta = c['th'].mean(axis=0)
    starts = dict(lo=[-0.05, -0.05], hi=[0.05, 0.05], seed=seed)

    def run(ctx, feed):
        out = {}
        ctx.set_step_sizes(np.full(ctx.n_params, alpha, np.float32))
        ctx.switch_to_pre_update()
        for step in (0, 1):
            feed(ctx, step, out)
            ctx.process_samples(step, **opts)
            proc = ctx.download_processed(step)
            out['ret%d' % step], out['adv%d' % step] = np.array(proc['returns']), np.array(proc['advantages'])
            if step == 0:
                ctx.inner_adapt(0)
                out['adapted'] = ctx.get_task_thetas()
        res = ctx.optimize(1, 1e-3, 0.3, eta)
        out.update(loss_before=res['loss_before'], loss_after=res['loss_after'], inner_kl=res['inner_kl'], outer_kl=res['outer_kl'],
                   theta=ctx.get_theta())
        return out

    def collect(ctx, step, out):
        out['tables%d' % step] = ctx.collect_point_family(step, 'goal', c['tasks'], None, None, total_samples=c['total'], max_path_length=T,
                                                          clip_infos=True, seed=seed, starts=starts, envs_per_task=B, max_steps=c['S'],
                                                          **c['env'])
        out['slab%d' % step] = ctx.download_step(step)

    def upload(ctx, step, out):
        t, s = dev['tables%d' % step], dev['slab%d' % step]
        ctx.upload_step(step, t['task_path_offsets'], t['path_row_offsets'], s['obs'], s['rew'], s['act'], s['old_mean'], s['old_log_std'])

    rows = c['S'] * M * B
    results = []
    for feed in (collect, upload):
        ctx = _lib.Context(M, 2, 2, hidden, 1, max_rows=rows, max_paths=rows, lib=lib)
        try:
            ctx.set_min_std(MIN_STD)
            ctx.set_theta(theta)
            results.append(run(ctx, feed))
            dev = results[0]
        finally:
            ctx.close()
    dev, host = results
    t0 = dev['tables0']
    first = dev['slab0']['obs'][t0['path_row_offsets'][:-1]]
    want = ps.start_rows(seed, 0, t0['path_start'].astype(np.int64) * M * B + t0['path_env'], 2, starts['lo'], starts['hi'])
    assert np.array_equal(first, want.astype(np.float32))
    assert len(set(t0['path_len'])) > 1, 'the case is not ragged'
    assert np.any(dev['adapted'] != theta[None, :]) and np.any(dev['theta'] != theta)
    for k in ('ret0', 'adv0', 'ret1', 'adv1', 'adapted', 'loss_before', 'loss_after', 'inner_kl', 'outer_kl', 'theta'):
        np.testing.assert_allclose(dev[k], host[k], rtol=1e-6, atol=1e-7, err_msg=k)
