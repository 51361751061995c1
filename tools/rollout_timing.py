"""Developer measurement for SURVEY 8f rows 1/3, rollout collection on the point-mass meta-environments.

    python tools/rollout_timing.py                       env-steps/s of a sampling step, host loop (MetaSampler: one device policy
                                                         query per environment step) vs device rollout (DevicePointEnvSampler)
    python tools/rollout_timing.py --launch [--kinds corner walls momentum] [--lib PATH] [--repeats N] [--launches W]
                                                         time of ONE rollout launch through the C ABI (upload of tasks, start states
                                                         and host noise + the kernel, ended by a device synchronise), per kind and
                                                         noise mode, at BASELINE config 1's shapes: median and spread over N windows
                                                         of W launches.  --lib binds another build of the library (an A/B against
                                                         another commit: run the two alternately in one job); corner goes through
                                                         promp_rollout_point_env, which every build has.
    python tools/rollout_timing.py --launch --wide ...   the same at 40 tasks and a 2x64 MLP (M 40, B 20, T 100), corner through
                                                         promp_rollout_point_family
    python tools/rollout_timing.py --launch --collect [--kinds corner goal] ...
                                                         time of ONE promp_collect_point_family call at M 40, B 20, T 100, (64,64):
                                                         max_steps = 2 T - 1 = 199 vectorised steps, total_samples = M B T, the
                                                         start table [199][800][2] float64 uploaded with every call; also per
                                                         vectorised step, beside which `--wide` puts the fixed-horizon launch's
                                                         time per step (its T = 100 steps).
    python tools/rollout_timing.py --launch --collect --normalize [--kinds corner goal] ...
                                                         the same call through promp_collect_point_family_norm with the normalize
                                                         wrapper's running moments off (the plain kernels), on the observations, and
                                                         on observations and rewards: what staging the moments behind every step
                                                         ([199][2 O + 2][800] float64) and the commit launch cost.  A --lib from before
                                                         the entry point runs the plain call only.
    python tools/rollout_timing.py --launch --collect [--normalize] --device-starts [--kinds corner goal]
                                                         the same calls through promp_collect_point_family_dev: every reset() drawn on
                                                         the device from the class's box (corner +-0.2, goal lo = hi = 0), no start
                                                         table reserved or uploaded.  Not with a --lib from before the entry point.
    python tools/rollout_timing.py --sampler-starts [--kinds goal origin corner]
                                                         host time of one DevicePointEnvSampler.obtain_samples at M 40, B 20, T 100,
                                                         (64,64) with device noise, start states from NumPy against device_starts=True:
                                                         where the host's draw of the start table shows."""
import argparse
import sys
import time

import numpy as np

sys.path.insert(0, '.')


def sampler_rates():
    from promp_amd.envs.point_env import make_point_env
    from promp_amd.policies.meta_gaussian_mlp_policy import MetaGaussianMLPPolicy
    from promp_amd.samplers.device_point_sampler import DevicePointEnvSampler
    from promp_amd.samplers.meta_sampler import MetaSampler
    for kind in ('corner', 'walls', 'momentum'):
        for M, B, T in ((4, 20, 100), (40, 20, 200)):
            np.random.seed(0)
            env = make_point_env(kind)
            policy = MetaGaussianMLPPolicy(name='p', obs_dim=int(np.prod(env.observation_space.shape)), action_dim=2, meta_batch_size=M,
                                           hidden_sizes=(32, 32))
            policy.switch_to_pre_update()
            for name, cls, reps in (('host loop   ', MetaSampler, 2), ('device kernel', DevicePointEnvSampler, 20)):
                s = cls(env=env, policy=policy, rollouts_per_meta_task=B, meta_batch_size=M, max_path_length=T)
                s.update_tasks()
                s.obtain_samples()
                t0 = time.time()
                for _ in range(reps):
                    s.obtain_samples()
                dt = (time.time() - t0) / reps
                print('%-8s M=%d B=%d T=%d  %s %9.3f ms per sampling step  %12.0f env-steps/s' % (
                    kind, M, B, T, name, 1e3 * dt, M * B * T / dt))


def bind(lib_path, kinds, need_family=False):
    """the library, or another build of it: entry points a build from before them lacks are left unbound"""
    from promp_amd import _lib
    if not lib_path:
        return _lib.Library()
    newest = ['promp_collect_point_family_dev', 'promp_rollout_point_family_dev', 'promp_draw_point_starts',
              'promp_collect_point_family_norm', 'promp_point_norm_set', 'promp_point_norm_get', 'promp_collect_point_family',
              'promp_rollout_point_family']
    held = {}
    try:
        while True:
            try:
                return _lib.Library(lib_path)
            except AttributeError:
                name = newest.pop(0)                           # (raises IndexError when something else is missing)
                held[name] = _lib.SIGNATURES.pop(name)
                if name == 'promp_rollout_point_family':
                    assert kinds == ['corner'] and not need_family, 'this library has the corner environment only'
    finally:
        _lib.SIGNATURES.update(held)


def timed(run, ctx, repeats, launches, warm=20):
    for _ in range(warm):                                      # warm-up: code objects, buffers
        run()
    ctx.sync()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(launches):
            run()
        ctx.sync()
        times.append((time.perf_counter() - t0) / launches)
    return 1e6 * np.array(times)


def sampler_start_times(kinds, repeats, launches):
    from promp_amd.envs.normalized_env import normalize
    from promp_amd.envs.point_env import make_point_env
    from promp_amd.policies.meta_gaussian_mlp_policy import MetaGaussianMLPPolicy
    from promp_amd.samplers.device_point_sampler import DevicePointEnvSampler
    M, B, T, hidden = 40, 20, 100, (64, 64)
    for kind in kinds:
        for wrapper in (dict(), dict(normalize_obs=True, normalize_reward=True)):
            for device_starts in (False, True):
                np.random.seed(0)
                env = normalize(make_point_env(kind), **wrapper)
                policy = MetaGaussianMLPPolicy(name='p', obs_dim=int(np.prod(env.observation_space.shape)), action_dim=2,
                                               meta_batch_size=M, hidden_sizes=hidden)
                policy.switch_to_pre_update()
                s = DevicePointEnvSampler(env=env, policy=policy, rollouts_per_meta_task=B, meta_batch_size=M, max_path_length=T,
                                          envs_per_task=B, device_noise=True, device_starts=device_starts)
                s.update_tasks()
                s.obtain_samples()
                times = []
                for _ in range(repeats):
                    t0 = time.perf_counter()
                    for _ in range(launches):
                        s.obtain_samples()
                    times.append((time.perf_counter() - t0) / launches)
                ms = 1e3 * np.array(times)
                print('obtain_samples %-8s %-10s device_starts %-5s  median %9.3f ms  min %9.3f  max %9.3f  (%d windows of %d calls)' % (
                    kind, 'normalised' if wrapper else 'plain', device_starts, np.median(ms), ms.min(), ms.max(), repeats, launches),
                    flush=True)


def collect_times(kinds, lib_path, repeats, launches, label, normalize=False, device_starts=False):
    from promp_amd import _lib, synthetic
    M, B, T, hidden = 40, 20, 100, (64, 64)
    S, N = 2 * T - 1, M * B
    lib = bind(lib_path, kinds)
    rng = np.random.RandomState(0)
    for kind in kinds:
        task_dim, O = _lib.POINT_KIND_DIMS[kind]
        ctx = _lib.Context(M, O, 2, hidden, 1, max_rows=S * N, max_paths=S * N, lib=lib)
        ctx.set_theta(synthetic.init_theta(rng, O, hidden, 2))
        ctx.switch_to_pre_update()
        if kind == 'goal':                                     # MetaPointEnvV2: goals in the square, every episode from the origin
            tasks, start, max_step = rng.uniform(-2, 2, size=(M, 2)), np.zeros((S, N, O)), 0.1
        else:
            tasks, start, max_step = rng.randn(M, task_dim), rng.uniform(-0.2, 0.2, size=(S, N, O)), 0.2 if kind != 'momentum' else 0.1
        z = rng.randn(S, N, 2).astype(np.float32)
        out = {}
        # device starts: the box the table above was drawn from; no table is handed over
        half = 0.0 if kind == 'goal' else 0.2
        dev = dict(starts=dict(lo=[-half] * O, hi=[half] * O, seed=12345), envs_per_task=B, max_steps=S) if device_starts else {}
        if normalize:
            norm_times(ctx, lib, kind, tasks, start, z, max_step, S, N, T, O, repeats, launches, label, dev)
            ctx.close()
            continue
        for noise in ('host', 'device'):
            def run():
                out['t'] = ctx.collect_point_family(0, kind, tasks, None if dev else start, z if noise == 'host' else None,
                                                    total_samples=N * T, max_path_length=T, seed=12345, reward_type='dense',
                                                    normalization_scale=10.0, max_step=max_step, **dev)
            us = timed(run, ctx, repeats, launches, warm=5)
            t = out['t']
            print('%scollect %-8s %-6s noise  median %9.2f us per call  min %9.2f  max %9.2f  = %7.2f us per vectorised step (%d steps); '
                  'stop step %d, %d paths, %d rows  (%d windows of %d calls)' % (
                      label, kind, noise, np.median(us), us.min(), us.max(), np.median(us) / S, S, t['n_steps'] - 1, len(t['path_len']),
                      t['path_row_offsets'][-1], repeats, launches), flush=True)
        ctx.close()


def norm_times(ctx, lib, kind, tasks, start, z, max_step, S, N, T, O, repeats, launches, label, dev):
    """host noise; plain: promp_collect_point_family; off / obs / both: promp_collect_point_family_norm with a start table one row
    longer.  The moments start as a fresh wrapper's and move on from call to call (step sizes 0.001, the wrapper's default)."""
    modes = [('plain', None)]
    longer = None
    if hasattr(lib.cdll, 'promp_collect_point_family_norm'):
        modes += [(name, dict(normalize_obs=n_obs, normalize_reward=n_rew, obs_alpha=0.001, reward_alpha=0.001))
                  for name, n_obs, n_rew in (('off', False, False), ('obs', True, False), ('both', True, True))]
        longer = np.concatenate([start, start[:1]])
        fresh = np.tile(np.concatenate([np.zeros(O), np.ones(O), [0.0, 1.0]]), (N, 1))
        ctx.set_point_norm(fresh)
    out = {}
    for name, norm in modes:
        def run():
            table = None if dev else start if norm is None else longer
            out['t'] = ctx.collect_point_family(0, kind, tasks, table, z, total_samples=N * T, max_path_length=T, seed=12345,
                                                reward_type='dense', normalization_scale=10.0, max_step=max_step, norm=norm, **dev)
        us = timed(run, ctx, repeats, launches, warm=5)
        t = out['t']
        print('%scollect %-8s normalize %-5s  median %9.2f us per call  min %9.2f  max %9.2f  = %7.2f us per vectorised step (%d steps); '
              'stop step %d, %d paths, %d rows; staged moments %.2f MB  (%d windows of %d calls)' % (
                  label, kind, name, np.median(us), us.min(), us.max(), np.median(us) / S, S, t['n_steps'] - 1, len(t['path_len']),
                  t['path_row_offsets'][-1], (8e-6 * S * (2 * O + 2) * N) if norm and (norm['normalize_obs'] or norm['normalize_reward']) else 0.0,
                  repeats, launches), flush=True)


def launch_times(kinds, lib_path, repeats, launches, label, wide=False):
    from promp_amd import _lib, synthetic
    M, B, T, hidden = (40, 20, 100, (64, 64)) if wide else (4, 20, 100, (32, 32))     # BASELINE config 1 (wide: 40 tasks, 2x64)
    lib = bind(lib_path, kinds, need_family=wide)
    rng = np.random.RandomState(0)
    for kind in kinds:
        task_dim, O = _lib.POINT_KIND_DIMS[kind]
        ctx = _lib.Context(M, O, 2, hidden, 1, max_rows=M * B * T, max_paths=M * B, lib=lib)
        ctx.set_theta(synthetic.init_theta(rng, O, hidden, 2))
        ctx.switch_to_pre_update()
        tasks, start = rng.randn(M, task_dim), rng.uniform(-0.2, 0.2, size=(M, B, O))
        z = rng.randn(M, B, T, 2).astype(np.float32)
        env = dict(reward_type='dense', normalization_scale=10.0, max_step=0.2 if kind != 'momentum' else 0.1)
        for noise in ('host', 'device'):
            kw = dict(noise=z if noise == 'host' else None, seed=12345, path_length=T, **env)
            if kind == 'corner' and not wide:
                run = lambda: ctx.rollout_point_env(0, tasks, start, **kw)
            else:
                run = lambda: ctx.rollout_point_family(0, kind, tasks, start, **kw)
            us = timed(run, ctx, repeats, launches)
            per_step = '  = %7.2f us per step (%d steps)' % (np.median(us) / T, T) if wide else ''
            print('%s%-8s %-6s noise  median %8.2f us per launch  min %8.2f  max %8.2f%s  (%d windows of %d launches)' % (
                label, kind, noise, np.median(us), us.min(), us.max(), per_step, repeats, launches), flush=True)
        ctx.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--launch', action='store_true')
    ap.add_argument('--collect', action='store_true')
    ap.add_argument('--wide', action='store_true')
    ap.add_argument('--normalize', action='store_true')
    ap.add_argument('--device-starts', action='store_true')
    ap.add_argument('--sampler-starts', action='store_true')
    ap.add_argument('--kinds', nargs='+', default=None, choices=['corner', 'walls', 'momentum', 'goal', 'origin'])
    ap.add_argument('--lib', type=str, default='')
    ap.add_argument('--label', type=str, default='')
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--launches', type=int, default=300)
    args = ap.parse_args()
    label = args.label and args.label + ' '
    if args.device_starts:
        assert args.launch and args.collect, '--device-starts goes with --launch --collect [--normalize] [--lib PATH]'
    if args.sampler_starts:
        sampler_start_times(args.kinds or ['goal', 'origin', 'corner'], args.repeats, args.launches)
    elif args.launch and args.collect:
        collect_times(args.kinds or ['corner', 'goal'], args.lib, args.repeats, args.launches, label, args.normalize, args.device_starts)
    elif args.launch:
        launch_times(args.kinds or ['corner', 'walls', 'momentum'], args.lib, args.repeats, args.launches, label, args.wide)
    else:
        sampler_rates()
