"""Device collections whose episodes end early (promp_collect_point_family; MetaPointEnv and MetaPointEnvV2), shared by
test_point_collect_host.py (CPU), test_emu_point_collect.py (emulator, tiny) and test_gpu_point_collect.py (MI355X).  Through the C
ABI, in the style of tests/point_family_checks.py, whose inputs (rollout_checks.make_thetas), replay (forward32) and bound rule are
used as they are.

`goal_step` restates the goal kind in float64 NumPy: s' = s + move, reward -|s' - goal|, done = |s'_0| < r and |s'_1| < r around the
ORIGIN; it is pinned by tests/golden/point_env_{origin,goal}.npz, outputs of the reference's two classes
(tools/gen_point_term_golden.py).  `collect_oracle` is the reference's sampler loop (samplers/meta_sampler.py:87-130 +
vectorized_env_executor.py:25-52) on a start table and a noise table: every environment steps in lock step, an episode ends when
the environment says so or at max_path_length, the environment continues from start[s + 1][env], collection stops at the first
step after which total_samples steps lie in finished episodes, and the finished episodes are listed per task by the step they end
at, then by environment.  test_point_collect_host.py pins it against the package's own MetaSampler driving the NumPy class.

Termination is discontinuous, so the checks are split as for walls:
  * TABLES: exact equality with the free-running float64 oracle, under the condition -- on the oracle's trajectory alone -- that
    every `done` comparison it evaluated lies at least MARGIN_FREE from a tie, MARGIN_FREE = 100 x the largest deviation of the
    float32 replay's observations (rollout_checks.forward32, one fmaf for the action) from the oracle's on that case, computed on
    the CPU.  The kernel's output never enters a bound.
  * SLAB: by induction per listed path.  A path starts from start[path_start][env], so paths are independent: obs[t] against
    float32(state_t) at ATOL; mean[t] against the oracle network at the stored obs[t], act[t] against that mean + exp(log_std) *
    noise, both by the bound rule; (state, reward, done) = goal_step(state, act[t] AS STORED); the reward at ATOL; done False before
    the last row; done True or length = max_path_length at the last row; every box comparison with margin >= MARGIN.
Each case asserts, on the oracle's trajectory alone, that the events it exists for occur (EVENTS below); data_seed is chosen on the
CPU so that they do.  Nothing is masked or skipped.

Inputs: starts within +-0.05 of the origin, exploration scaled so that one step moves the point by about the box's half-width
(log_std around log 0.8 under the wrapper's scale 10, where a policy unit is 0.01; the bare environment takes log_std around
log 0.008 and the output layer scaled by 0.01), so the walk crosses the box often.
"""
import os

import numpy as np

from oracle import philox, policy as op
from promp_amd import _lib
from tests import helpers, point_family_checks as fc, rollout_checks as rc
from tests.rollout_checks import ATOL, ATOL_DEVICE_NOISE, ATOL_LOG_STD, MIN_STD, SEED31, SEED64, bound, maxdev

MARGIN = 1e-9
DONE_RADIUS = 0.01
MAX_STEP = 0.1
# what a case can be built for; check_goal_collect asserts the ones it is given on the oracle's trajectory
EVENTS = ('length_1', 'horizon', 'three_episodes', 'stop_beyond_T', 'rows_exceed', 'dropped_tail', 'unequal_counts', 'done')


# ---- the environment, float64 ---------------------------------------------------------------------------------------------------

def goal_step(state, action, goal, normalization_scale, max_step=MAX_STEP, done_radius=DONE_RADIUS):
    """one step for a batch: state [n, 2], action [n, 2] (policy scale), goal [2] or [n, 2] -> (next state, reward [n], done [n],
    margin [n]: the smallest distance of an evaluated box comparison from a tie -- `a and b` stops at a false a)"""
    state = np.asarray(state, dtype=np.float64)
    nxt = state + fc._move(action, normalization_scale, max_step)
    d = nxt - np.asarray(goal, dtype=np.float64)
    rew = -np.sqrt(np.sum(d * d, axis=-1))
    in0, in1 = np.abs(nxt[:, 0]) < done_radius, np.abs(nxt[:, 1]) < done_radius
    m0, m1 = np.abs(np.abs(nxt[:, 0]) - done_radius), np.abs(np.abs(nxt[:, 1]) - done_radius)
    return nxt, rew, in0 & in1, np.where(in0, np.minimum(m0, m1), m0)


def load_fixture(name):
    return np.load(os.path.join(helpers.GOLDEN, 'point_env_%s.npz' % name))


def make_env(name, normalization_scale):
    """the package's NumPy class, wrapped as the fixture's trajectory was"""
    from promp_amd.envs import point_env
    from promp_amd.envs.normalized_env import normalize
    bare = dict(origin=point_env.MetaPointEnv, goal=point_env.MetaPointEnvV2)[name]()
    return (normalize(bare) if normalization_scale > 0 else bare), bare


# ---- the collection oracle --------------------------------------------------------------------------------------------------------

def policy_actions(spec, th, obs32, z, B, f32=False):
    """obs32 [M * B, 2] float32, z [M * B, 2] -> (mean, action) under every task's own parameters; f32: as the kernels compute them"""
    M = len(th)
    mean, act = np.zeros((M * B, 2), np.float32 if f32 else np.float64), np.zeros((M * B, 2), np.float32 if f32 else np.float64)
    for i in range(M):
        rows = slice(i * B, (i + 1) * B)
        if f32:
            mean[rows] = rc.forward32(spec, th[i], obs32[rows])
            act[rows] = helpers.fma32(np.exp(th[i, -2:].astype(np.float32)).astype(np.float32)[None, :], z[rows], mean[rows])
        else:
            mean[rows] = op.forward(spec, th[i].astype(np.float64), obs32[rows].astype(np.float64), False)[0]
            act[rows] = mean[rows] + np.exp(th[i, -2:].astype(np.float64)) * z[rows]
    return mean, act


def tables_of(end_len, M, B, total_samples):
    """end_len [S, M * B] -> None if total_samples is not reached, else dict(stop, rows, tpo, env, start, len): the reference's
    loop over a finished end_len table"""
    S = end_len.shape[0]
    total, per_task = 0, [[] for _ in range(M)]
    for s in range(S):
        for env in np.flatnonzero(end_len[s] > 0):
            n = int(end_len[s, env])
            per_task[env // B].append((int(env), s - n + 1, n))
            total += n
        if total >= total_samples:
            flat = [p for tp in per_task for p in tp]
            return dict(stop=s, rows=total, tpo=np.concatenate([[0], np.cumsum([len(tp) for tp in per_task])]).astype(np.int32),
                        env=np.array([p[0] for p in flat], np.int32), start=np.array([p[1] for p in flat], np.int32),
                        len=np.array([p[2] for p in flat], np.int32))
    return None


def collect_oracle(spec, th, tasks, start, z, B, T, total_samples, step, f32=False):
    """start [S, M * B, 2], z [S, M * B, 2], tasks [M, 2]; step(state, action, goals [n, 2]) -> (next, reward, done, margin).
    Runs all S steps (as the device does) -> dict(obs, mean, act, rew [S, n, ..] staging rows, end_len [S, n], margin: the smallest
    done margin up to the stop step, tables: tables_of(...))"""
    S, N = start.shape[:2]
    M = len(th)
    goals = np.repeat(np.asarray(tasks, np.float64), B, axis=0)
    dt = np.float32 if f32 else np.float64
    obs, mean, act = np.zeros((S, N, 2), np.float32), np.zeros((S, N, 2), dt), np.zeros((S, N, 2), dt)
    rew, end_len, margins = np.zeros((S, N)), np.zeros((S, N), np.int32), np.zeros((S, N))
    state, length = np.asarray(start[0], np.float64).copy(), np.zeros(N, np.int64)
    for s in range(S):
        obs[s] = state.astype(np.float32)
        mean[s], act[s] = policy_actions(spec, th, obs[s], z[s], B, f32)
        nxt, rew[s], done, margins[s] = step(state, act[s].astype(np.float32).astype(np.float64), goals)
        length += 1
        end = done | (length >= T)
        end_len[s] = np.where(end, length, 0)
        length[end] = 0
        state = np.where(end[:, None], start[s + 1], nxt) if s + 1 < S else nxt
    tables = tables_of(end_len, M, B, total_samples)
    upto = (tables['stop'] + 1) if tables else S
    return dict(obs=obs, mean=mean, act=act, rew=rew, end_len=end_len, margin=float(margins[:upto].min()), tables=tables)


def gather(stage, tables):
    """the staging rows of the listed paths, in path order"""
    s = np.concatenate([s0 + np.arange(n) for s0, n in zip(tables['start'], tables['len'])])
    e = np.concatenate([np.full(n, e) for e, n in zip(tables['env'], tables['len'])])
    return stage[s, e]


def events_of(o, M, B, T, total_samples):
    """the events of EVENTS that occur on the oracle collection o"""
    t = o['tables']
    stop = t['stop']
    found = set()
    if (t['len'] == 1).any():
        found.add('length_1')
    if (t['len'] == T).any():
        found.add('horizon')
    if (t['len'] < T).any():
        found.add('done')
    if np.bincount(t['env'], minlength=M * B).max() >= 3:
        found.add('three_episodes')
    if stop >= T:
        found.add('stop_beyond_T')
    if t['rows'] > total_samples:
        found.add('rows_exceed')
    if (o['end_len'][stop] == 0).any():            # an environment was in the middle of an episode when collection stopped
        found.add('dropped_tail')
    if len(set(np.diff(t['tpo']))) > 1:
        found.add('unequal_counts')
    return found


# ---- cases ------------------------------------------------------------------------------------------------------------------------

def max_steps_of(M, B, T, total_samples):
    return T - 1 + -(-total_samples // (M * B))


def goal_case(M, B, T, hidden, normalization_scale, noise, step, seed, data_seed=0, rollouts=None, origin=False):
    """rollouts: rollouts_per_meta_task (total_samples = M * rollouts * T), default B; origin: every goal (0, 0), MetaPointEnv"""
    rng = np.random.RandomState(7000 + data_seed)
    spec = op.PolicySpec(2, 2, hidden, min_std=MIN_STD)
    th = rc.make_thetas(rng, M, 2, 2, hidden)
    unit = 0.01 if normalization_scale > 0 else 1.0            # what one policy unit moves the point by
    th[:, -2:] = (np.log(0.008 / unit) + rng.uniform(-0.3, 0.3, size=(M, 2))).astype(np.float32)
    for i in range(M if normalization_scale > 0 else 0):       # one entry of every task below log(MIN_STD): the clip modes differ
        th[i, -2 + i % 2] = np.float32(np.log(MIN_STD) - 0.1 - 0.05 * i)
    if normalization_scale == 0:                               # the bare environment: means of the box's size (all of its log_std
                                                               # lie below the floor)
        n_out = hidden[-1] * 2 + 2
        th[:, -(n_out + 2):-2] *= np.float32(0.01)
    tasks = np.zeros((M, 2)) if origin else rng.uniform(-2, 2, size=(M, 2))
    total = M * (rollouts or B) * T
    S = max_steps_of(M, B, T, total)
    start = rng.uniform(-0.05, 0.05, size=(S, M * B, 2))
    if noise == 'host':
        z = rng.randn(S, M * B, 2).astype(np.float32)
    else:                                                      # the staging row is the counter
        z = rc.assert_noise_depends_on_high_word_and_stream(seed, np.arange(S * M * B), 2, step).reshape(S, M * B, 2)
    env = dict(normalization_scale=float(normalization_scale), max_step=MAX_STEP, done_radius=DONE_RADIUS)
    return dict(spec=spec, hidden=hidden, th=th, tasks=tasks, start=start, z=z, env=env, M=M, B=B, T=T, total=total, S=S, noise=noise)


def case_oracle(c, f32=False):
    step = lambda state, action, goals: goal_step(state, action, goals, c['env']['normalization_scale'])
    return collect_oracle(c['spec'], c['th'], c['tasks'], c['start'], c['z'], c['B'], c['T'], c['total'], step, f32)


def case_conditions(c, wanted):
    """CPU only, on the oracle alone -> (oracle collection, MARGIN_FREE): the events the case is built for occur, the free-running
    tables are decidable (margin >= MARGIN_FREE), and the reported log_std differs between the two clip modes"""
    o = case_oracle(c)
    assert o['tables'] is not None, 'the oracle does not reach total_samples'
    found = events_of(o, c['M'], c['B'], c['T'], c['total'])
    assert set(wanted) <= set(EVENTS) and set(wanted) <= found, (sorted(wanted), sorted(found))
    r32 = case_oracle(c, f32=True)
    upto = o['tables']['stop'] + 1
    margin_free = 100.0 * maxdev(r32['obs'][:upto], o['obs'][:upto])
    assert margin_free < DONE_RADIUS / 10, margin_free          # (a replay that took another branch would show here)
    assert o['margin'] >= max(margin_free, MARGIN), (o['margin'], margin_free)
    return o, margin_free


def open_context(lib, c, K=1):
    rows = c['S'] * c['M'] * c['B']
    ctx = _lib.Context(c['M'], 2, 2, c['hidden'], K, max_rows=rows, max_paths=rows, lib=lib)
    ctx.set_min_std(MIN_STD)
    ctx.set_theta(c['th'].mean(axis=0))
    ctx.set_task_thetas(c['th'])
    return ctx


def collect_device(ctx, c, step, seed, clip_infos, kind='goal', **over):
    kw = dict(total_samples=c['total'], max_path_length=c['T'], clip_infos=clip_infos, seed=seed, **c['env'])
    kw.update(over)
    z = c['z'][:len(c['start'])] if c['noise'] == 'host' else None
    return ctx.collect_point_family(step, kind, c['tasks'], c['start'], z, **kw)


def assert_tables(got, want, M):
    assert got['n_steps'] == want['stop'] + 1, (got['n_steps'], want['stop'] + 1)
    for k_got, k_want in (('task_path_offsets', 'tpo'), ('path_env', 'env'), ('path_start', 'start'), ('path_len', 'len')):
        assert got[k_got].dtype == np.int32 and np.array_equal(got[k_got], want[k_want]), (k_got, got[k_got], want[k_want])
    assert np.array_equal(got['path_row_offsets'], np.concatenate([[0], np.cumsum(want['len'])]))
    assert got['task_path_offsets'].shape == (M + 1,)


def slab_induction(c, tables, slab, verbose=''):
    """the induction of the module docstring over the listed paths, all paths abreast -> (errors, bounds, smallest margin)"""
    spec, th, B, T = c['spec'], c['th'], c['B'], c['T']
    env, s0, ln = tables['path_env'], tables['path_start'], tables['path_len']
    pro = tables['path_row_offsets']
    assert slab['obs'].shape == (pro[-1], 2) and slab['rew'].shape == (pro[-1],)
    goals = np.asarray(c['tasks'], np.float64)[env // B]
    atol_act = ATOL if c['noise'] == 'host' else ATOL_DEVICE_NOISE
    state = np.asarray(c['start'], np.float64)[s0, env]
    err, margin = dict(obs=0.0, mean=0.0, act=0.0, rew=0.0), np.inf
    tol_mean, tol_act = ATOL, atol_act
    for t in range(int(ln.max())):
        live = np.flatnonzero(ln > t)
        rows = pro[live] + t
        obs, act, mean = slab['obs'][rows], slab['act'][rows], slab['old_mean'][rows]
        err['obs'] = max(err['obs'], maxdev(obs, state[live].astype(np.float32)))
        z = c['z'][s0[live] + t, env[live]]
        for i in range(c['M']):
            sel = env[live] // B == i
            if not sel.any():
                continue
            m_ref = op.forward(spec, th[i].astype(np.float64), obs[sel].astype(np.float64), False)[0]
            m32 = rc.forward32(spec, th[i], obs[sel])
            a_ref = m_ref + np.exp(th[i, -2:].astype(np.float64)) * z[sel]
            a32 = helpers.fma32(np.exp(th[i, -2:]).astype(np.float32)[None, :], z[sel], m32)
            tol_mean, tol_act = max(tol_mean, bound(ATOL, maxdev(m32, m_ref))), max(tol_act, bound(atol_act, maxdev(a32, a_ref)))
            err['mean'] = max(err['mean'], maxdev(mean[sel], m_ref))
            err['act'] = max(err['act'], maxdev(act[sel], a_ref))
        nxt, r, done, mg = goal_step(state[live], act.astype(np.float64), goals[live], c['env']['normalization_scale'])
        err['rew'] = max(err['rew'], maxdev(slab['rew'][rows], r))
        margin = min(margin, float(mg.min()))
        last = ln[live] == t + 1
        assert not done[~last].any(), 'an episode went on behind a done'
        assert (done[last] | (ln[live][last] == T)).all(), 'an episode ends without a done before max_path_length'
        state[live] = nxt
    tol = dict(obs=ATOL, mean=tol_mean, act=tol_act, rew=ATOL)
    print('%s %d paths, margin %.2e; bounds %s; device %s' % (verbose, len(ln), margin, {k: '%.2e' % v for k, v in tol.items()},
                                                              {k: '%.2e' % v for k, v in err.items()}))
    return err, tol, margin


def check_goal_collect(lib, M, B, T, hidden, normalization_scale, noise, step, seed, clip_infos, wanted, data_seed=0, rollouts=None,
                       origin=False):
    c = goal_case(M, B, T, hidden, normalization_scale, noise, step, seed, data_seed, rollouts, origin)
    o, margin_free = case_conditions(c, wanted)
    ctx = open_context(lib, c)
    try:
        got = collect_device(ctx, c, step, seed, clip_infos)
        slab = ctx.download_step(step)
    finally:
        ctx.close()
    want = o['tables']
    print('goal %s %s scale %g %s step %d: stop %d rows %d of %d, %d paths %s, oracle margin %.2e >= %.2e' % (
        (M, B, T), hidden, normalization_scale, noise, step, want['stop'], want['rows'], c['total'], len(want['len']),
        np.diff(want['tpo']).tolist(), o['margin'], margin_free))
    assert_tables(got, want, M)
    err, tol, margin = slab_induction(c, got, slab, 'goal %s %s:' % ((M, B, T), hidden))
    assert margin >= MARGIN, margin
    for k in ('obs', 'mean', 'act', 'rew'):
        assert err[k] <= tol[k], (k, err[k], tol[k])
    np.testing.assert_allclose(slab['old_log_std'], rc.reported_log_std(c['th'], 2, clip_infos), rtol=0, atol=ATOL_LOG_STD)


def goal_case_is_sound(M, B, T, hidden, normalization_scale, noise, step, seed, clip_infos, wanted, data_seed=0, rollouts=None,
                       origin=False):
    """CPU only: the case's conditions, and the induction on the float32 replay's own free-running collection"""
    c = goal_case(M, B, T, hidden, normalization_scale, noise, step, seed, data_seed, rollouts, origin)
    o, margin_free = case_conditions(c, wanted)
    r32 = case_oracle(c, f32=True)
    t = r32['tables']
    for k in ('stop', 'rows'):
        assert t[k] == o['tables'][k]
    for k in ('tpo', 'env', 'start', 'len'):
        assert np.array_equal(t[k], o['tables'][k]), k
    tables = dict(path_env=t['env'], path_start=t['start'], path_len=t['len'], path_row_offsets=np.concatenate([[0], np.cumsum(t['len'])]))
    slab = dict(obs=gather(r32['obs'], t), act=gather(r32['act'], t), old_mean=gather(r32['mean'], t),
                rew=gather(r32['rew'], t).astype(np.float32))
    err, tol, margin = slab_induction(c, tables, slab)
    assert margin >= MARGIN
    for k in ('obs', 'mean', 'act', 'rew'):
        assert err[k] <= tol[k], (k, err[k], tol[k])
    return o


# ---- the table kernels on a hand-made end_len ------------------------------------------------------------------------------------

# [step][environment], M = 2, B = 3, max_path_length 5: two episodes end at step 3 (a tie at the stop step of total_samples = 9: both
# count, 15 rows); environment 4 finishes two episodes, the first of one step; environment 5 runs to the horizon; every
# environment but 5 has a running tail at step 3; with total_samples = 1 task 0 finishes nothing
HAND_END_LEN = np.array([[0, 0, 0, 0, 1, 0],
                         [0, 2, 0, 2, 0, 0],
                         [0, 0, 3, 0, 0, 0],
                         [4, 0, 0, 0, 3, 0],
                         [0, 3, 0, 0, 0, 5]], np.int32)
HAND_TABLES = dict(stop=3, rows=15, tpo=[0, 3, 6], env=[1, 2, 0, 4, 3, 4], start=[0, 0, 0, 0, 0, 1], len=[2, 3, 4, 1, 2, 3])


def hand_case():
    """inputs that realise HAND_END_LEN exactly: a zero network with log_std 0 makes the action the noise itself, the bare
    environment moves by it; every episode starts at (0.05, 0), stays there, and steps onto the origin when the table says so"""
    M, B, T = 2, 3, 5
    S, N = HAND_END_LEN.shape
    spec = op.PolicySpec(2, 2, (32, 32), min_std=MIN_STD)
    th = np.zeros((M, spec.n_params), np.float32)
    start = np.tile(np.array([0.05, 0.0]), (S, N, 1))
    z = np.zeros((S, N, 2), np.float32)
    z[..., 0] = np.where((HAND_END_LEN > 0) & (HAND_END_LEN < T), np.float32(-0.05), np.float32(0))
    env = dict(normalization_scale=0.0, max_step=MAX_STEP, done_radius=DONE_RADIUS)
    c = dict(spec=spec, hidden=(32, 32), th=th, tasks=np.array([[1.0, -1.0], [0.5, 2.0]]), start=start, z=z, env=env, M=M, B=B, T=T,
             total=9, S=S, noise='host')
    o = case_oracle(c)
    assert np.array_equal(o['end_len'], HAND_END_LEN) and o['margin'] > 1e-3
    for k, v in HAND_TABLES.items():
        assert np.array_equal(o['tables'][k], v), k
    return c, o


def check_hand_tables(lib):
    """k_collect_stop / k_collect_tables behind k_point_collect on HAND_END_LEN: the tables, the tie at the stop step, the gathered
    rows; a task that finishes nothing and max_steps one short are refused"""
    c, o = hand_case()
    ctx = open_context(lib, c)
    try:
        got = collect_device(ctx, c, 0, 0, False)
        slab = ctx.download_step(0)
        assert_tables(got, o['tables'], c['M'])
        t = o['tables']
        assert np.array_equal(slab['obs'], gather(o['obs'], t)) and np.array_equal(slab['act'], gather(o['act'], t).astype(np.float32))
        assert np.array_equal(slab['rew'], gather(o['rew'], t).astype(np.float32)) and slab['obs'].shape == (15, 2)
        # fewer samples: the stop step moves, the tables shrink; the same step again is the same tables (nothing left behind)
        for total in (5, 8, 9, 15):
            want = tables_of(HAND_END_LEN, c['M'], c['B'], total)
            assert_tables(collect_device(ctx, c, 1, 0, True, total_samples=total), want, c['M'])
            assert ctx.download_step(1)['obs'].shape == (want['rows'], 2)
        assert_tables(collect_device(ctx, c, 0, 0, True, total_samples=20), tables_of(HAND_END_LEN, c['M'], c['B'], 20), c['M'])
        for match, over in (('no finished episode for task(s) [0]', dict(total_samples=1)),
                            ('do not reach total_samples', dict(total_samples=24))):
            try:
                collect_device(ctx, c, 0, 0, True, **over)
            except _lib.PrompError as e:
                assert match in str(e), (match, str(e))
            else:
                raise AssertionError('accepted: expected a refusal naming %r' % match)
        try:
            collect_device(ctx, dict(c, start=c['start'][:3]), 0, 0, True)          # max_steps one short of the stop step
        except _lib.PrompError as e:
            assert 'do not reach total_samples' in str(e), str(e)
        else:
            raise AssertionError('accepted with max_steps one short')
    finally:
        ctx.close()


# ---- the fixed kinds, the stack, refusals -----------------------------------------------------------------------------------------

def check_fixed_kind_bitwise(lib, kind, M, B, T, hidden, reward_type, normalization_scale, step, clip_infos):
    """corner / momentum through promp_collect_point_family with host noise transposed to [s][env], total_samples = M B T: every
    episode ends by the horizon at step T - 1, so the slab is promp_rollout_point_family's bit for bit and the tables are p * T.
    Pins staging, stop step, ordering and gather at once."""
    if kind == 'corner':
        pc = rc.point_case(M, B, T, hidden, reward_type, normalization_scale, 'host', step, 0, clip_infos)
        c = dict(th=pc['th'], tasks=pc['goals'], start=pc['start'], z=pc['z'], env=pc['env'], hidden=hidden)
    else:
        c = fc.momentum_case(M, B, T, hidden, reward_type, normalization_scale, 'host', step, 0)
    O = fc.STATE_DIM[kind]
    ref = fc.run_device(lib, kind, c, step, 0, clip_infos, 'host')
    rng = np.random.RandomState(11)
    start = rng.uniform(-1, 1, size=(T, M * B, O))             # rows 1 .. T - 1 are never read: no episode ends before step T - 1
    start[0] = c['start'].reshape(M * B, O)
    z = np.ascontiguousarray(c['z'].reshape(M * B, T, 2).transpose(1, 0, 2))
    ctx = _lib.Context(M, O, 2, hidden, 1, max_rows=M * B * T, max_paths=M * B, lib=lib)
    try:
        ctx.set_min_std(MIN_STD)
        ctx.set_theta(c['th'].mean(axis=0))
        ctx.set_task_thetas(c['th'])
        got = ctx.collect_point_family(step, kind, c['tasks'], start, z, total_samples=M * B * T, max_path_length=T,
                                       clip_infos=clip_infos, **c['env'])
        slab = ctx.download_step(step)
    finally:
        ctx.close()
    assert got['n_steps'] == T
    assert np.array_equal(got['task_path_offsets'], np.arange(M + 1) * B) and np.array_equal(got['path_env'], np.arange(M * B))
    assert np.array_equal(got['path_start'], np.zeros(M * B)) and np.array_equal(got['path_row_offsets'], np.arange(M * B + 1) * T)
    assert np.any(ref['rew'] != 0) and np.all(np.isfinite(ref['act']))
    for k in ('obs', 'act', 'old_mean', 'rew', 'old_log_std'):
        assert slab[k].shape == ref[k].shape and np.array_equal(slab[k], ref[k]), k


def check_feeds_the_stack(lib, M, B, T, hidden, seed, data_seed=0):
    """collected goal slabs (steps 0 and 1, device noise) through process_samples, inner_adapt and one ProMP optimize, against the
    same paths uploaded from the host with promp_upload_step into a second context: resident == uploaded at the equality of
    test_plugin_api.run_device_rollout_scenario (rtol 1e-6, atol 1e-7)"""
    c = goal_case(M, B, T, hidden, 10, 'device', 0, seed, data_seed)
    alpha, eta = 0.1, np.array([5e-4], np.float32)
    opts = dict(discount=0.99, gae_lambda=1.0, normalize_adv=True)
    theta = c['th'].mean(axis=0)
    first = case_oracle(dict(c, th=np.tile(theta, (M, 1))))['tables']        # step 0 samples under theta itself
    assert len(set(first['len'])) > 1 and len(set(np.diff(first['tpo']))) > 1, 'the case is not ragged'

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
        c['z'] = philox.action_noise(seed, np.arange(c['S'] * M * B), 2, step).reshape(c['S'], M * B, 2)
        out['tables%d' % step] = collect_device(ctx, c, step, seed, True)
        out['slab%d' % step] = ctx.download_step(step)

    rows = c['S'] * M * B
    ctx = _lib.Context(M, 2, 2, hidden, 1, max_rows=rows, max_paths=rows, lib=lib)
    try:
        ctx.set_min_std(MIN_STD)
        ctx.set_theta(theta)
        dev = run(ctx, collect)
    finally:
        ctx.close()
    assert_tables(dev['tables0'], first, M)

    def upload(ctx, step, out):
        t, s = dev['tables%d' % step], dev['slab%d' % step]
        ctx.upload_step(step, t['task_path_offsets'], t['path_row_offsets'], s['obs'], s['rew'], s['act'], s['old_mean'], s['old_log_std'])

    ctx = _lib.Context(M, 2, 2, hidden, 1, max_rows=rows, max_paths=rows, lib=lib)
    try:
        ctx.set_min_std(MIN_STD)
        ctx.set_theta(theta)
        host = run(ctx, upload)
    finally:
        ctx.close()
    assert np.any(dev['adapted'] != theta[None, :]) and np.any(dev['theta'] != theta)
    for k in ('ret0', 'adv0', 'ret1', 'adv1', 'adapted', 'loss_before', 'loss_after', 'inner_kl', 'outer_kl', 'theta'):
        np.testing.assert_allclose(dev[k], host[k], rtol=1e-6, atol=1e-7, err_msg=k)


def check_refusals(lib):
    """by name, and with nothing installed: the step keeps no layout of the refused call"""
    c = goal_case(2, 3, 6, (32, 32), 10, 'host', 0, 0)
    o = case_oracle(c)
    rows = c['S'] * 6

    def refused(match, O=2, A=2, max_rows=rows, max_paths=rows, kind='goal', tasks=None, start=None, **over):
        ctx = _lib.Context(2, O, A, (32, 32), 1, max_rows=max_rows, max_paths=max_paths, lib=lib)
        cc = dict(c, tasks=c['tasks'] if tasks is None else tasks, start=c['start'] if start is None else start)
        try:
            ctx.set_task_thetas(np.zeros((2, ctx.n_params), np.float32))
            collect_device(ctx, cc, 0, 0, True, kind=kind, **over)
        except _lib.PrompError as e:
            assert match in str(e), (match, str(e))
            try:
                ctx.process_samples(0)
            except _lib.PrompError:
                pass
            else:
                raise AssertionError('the refused collection left data behind')
        else:
            raise AssertionError('accepted: expected a refusal naming %r' % match)
        finally:
            ctx.close()
    S = c['S']
    refused('do not reach total_samples', total_samples=S * 6 + 1)           # more than every staged step
    short = o['tables']['stop']                                               # one vectorised step short of the stop step
    refused('do not reach total_samples', start=c['start'][:short])
    refused('exceed max_rows', max_rows=o['tables']['rows'] - 1)
    refused('max_paths', max_paths=len(o['tables']['len']) - 1)
    refused('max_path_length', max_path_length=0)
    refused('unknown environment kind', kind=4)
    refused('unknown environment kind', kind=-1)
    refused('task_dim', kind=1)                                               # walls with a bare goal
    refused('task_dim', kind=3, tasks=np.zeros((2, 6)))                       # goal with walls' parameters
    refused('obs_dim', kind='momentum', O=2, start=np.zeros((S, 6, 4)))
    refused('obs_dim', kind='goal', O=4)
    refused('act_dim', kind='goal', A=3)
    # a task whose environments finish nothing before the others have filled total_samples: task 1 never comes near the box,
    # task 0 starts every episode in its middle (checked on the oracle)
    far = c['start'].copy()
    far[:, :3] *= 0.01
    far[:, 3:] += 1.0
    step = lambda state, action, goals: goal_step(state, action, goals, c['env']['normalization_scale'])
    t = collect_oracle(c['spec'], c['th'], c['tasks'], far, c['z'], 3, S + 1, 4, step)['tables']
    assert t is not None and t['tpo'][1] > 0 and t['tpo'][2] == t['tpo'][1]
    refused('no finished episode for task(s) [1]', start=far, max_path_length=S + 1, total_samples=4)


# ---- the sampler ------------------------------------------------------------------------------------------------------------------

def run_sampler_scenario(name, wrapped, M=3, B=3, R=4, T=10, hidden=(32, 32), device_noise=False):
    """DevicePointEnvSampler on MetaPointEnv ('origin') / MetaPointEnvV2 ('goal'), envs_per_task B below rollouts_per_meta_task R:
    ragged DevicePaths whose dict rows are the slab's, every path the NumPy class stepped on the RETURNED actions from
    start[path_start][env] (host noise: the sampler's draws replayed), process_samples uploads nothing.  The caller has bound the
    library (promp_amd._lib.set_library_for_testing)."""
    from promp_amd.baselines.linear_baseline import LinearFeatureBaseline
    from promp_amd.envs import point_env
    from promp_amd.envs.normalized_env import normalize
    from promp_amd.policies.meta_gaussian_mlp_policy import MetaGaussianMLPPolicy
    from promp_amd.samplers.device_point_sampler import DevicePointEnvSampler
    from promp_amd.samplers.meta_sample_processor import MetaSampleProcessor
    np.random.seed(29)
    bare = point_env.MetaPointEnv() if name == 'origin' else point_env.MetaPointEnvV2()
    env = normalize(bare) if wrapped else bare
    policy = MetaGaussianMLPPolicy(name='p', obs_dim=2, action_dim=2, meta_batch_size=M, hidden_sizes=hidden)
    sampler = DevicePointEnvSampler(env=env, policy=policy, rollouts_per_meta_task=R, meta_batch_size=M, max_path_length=T,
                                    envs_per_task=B, device_noise=device_noise)
    assert sampler.kind == name and sampler.envs_per_task == B and sampler.total_samples == M * R * T
    sampler.update_tasks()
    assert sampler.goals.shape == (M, 2) and (name == 'goal' or not sampler.goals.any())
    spec = op.PolicySpec(2, 2, hidden)
    theta = spec.from_ordered_dict(policy.get_param_values())
    theta[-2:] = np.log(0.8 if wrapped else 0.008)        # steps of about the box's half-width
    if not wrapped:
        theta[-(hidden[-1] * 2 + 4):-2] *= 0.01
    policy.set_params(spec.to_ordered_dict(theta))
    policy.switch_to_pre_update()
    state = np.random.get_state()
    paths = sampler.obtain_samples()
    np.random.set_state(state)                            # replay the sampler's draws
    S = max_steps_of(M, B, T, M * R * T)
    start = np.random.uniform(-2, 2, size=(S, M * B, 2)) if name == 'origin' else np.zeros((S, M * B, 2))
    fl = paths.flat
    tpo, pro, p_env, p_start = fl['task_path_offsets'], fl['path_row_offsets'], fl['path_env'], fl['path_start']
    assert list(paths.keys()) == list(range(M)) and [len(paths[i]) for i in range(M)] == np.diff(tpo).tolist()
    assert pro[-1] >= M * R * T and sampler.total_timesteps_sampled == M * R * T and paths.device_ref is not None
    lens, margin, p = np.diff(pro), np.inf, 0
    for i in range(M):
        env.set_task({} if name == 'origin' else sampler.goals[i])
        for path in paths[i]:
            rows = slice(pro[p], pro[p + 1])
            assert p_env[p] // B == i and path['observations'].shape == (lens[p], 2)
            for key, arr in (('observations', fl['obs']), ('actions', fl['act']), ('rewards', fl['rew'])):
                assert np.array_equal(path[key], arr[rows]), key
            assert np.array_equal(path['agent_infos']['mean'], fl['old_mean'][rows])
            assert np.array_equal(path['agent_infos']['log_std'], np.tile(fl['old_log_std'][i], (lens[p], 1)))
            env.reset()
            bare._state = start[p_start[p], p_env[p]].copy()
            s = bare._state
            for t in range(lens[p]):
                np.testing.assert_allclose(path['observations'][t], s.astype(np.float32), rtol=0, atol=ATOL)
                a = path['actions'][t].astype(np.float64)
                margin = min(margin, float(goal_step(s[None, :], a[None, :], sampler.goals[i], 10.0 if wrapped else 0.0)[3][0]))
                s, r, done, _ = env.step(a)
                np.testing.assert_allclose(path['rewards'][t], r, rtol=0, atol=ATOL)
                assert done == (t == lens[p] - 1) or (t == lens[p] - 1 and lens[p] == T), (p, t, done)
            mean = op.forward(spec, theta, path['observations'].astype(np.float64), False)[0]
            np.testing.assert_allclose(path['agent_infos']['mean'], mean, rtol=0, atol=ATOL)
            p += 1
    assert margin >= MARGIN                               # the NumPy class and the device saw the same side of every comparison
    if name == 'goal':
        assert len(set(lens)) > 1 and (lens < T).any()    # (from the origin with small steps: episodes do end early)
    # processing stays resident
    proc = MetaSampleProcessor(baseline=LinearFeatureBaseline(), discount=0.99, gae_lambda=1, normalize_adv=True)
    sess = policy.session
    counter, serial = sess._upload_counter, list(sess.upload_serial)
    sd = proc.process_samples(paths)
    assert sess._upload_counter == counter and sess.upload_serial == serial, 'device paths must not be uploaded again'
    assert len(sd) == M and sess.resident_slot(sd) is not None
    assert [len(s_['rewards']) for s_ in sd] == [int(pro[tpo[i + 1]] - pro[tpo[i]]) for i in range(M)]
    assert all(np.all(np.isfinite(np.asarray(s_['advantages']))) for s_ in sd)
