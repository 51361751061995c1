"""Device collections under the normalize wrapper's running observation / reward normalisation (promp_collect_point_family_norm,
promp_point_norm_set / _get), shared by test_point_norm_host.py (CPU), test_emu_point_norm.py (emulator, tiny),
test_gpu_point_norm.py and test_gpu_point_norm_sampler.py (MI355X).  Through the C ABI, in the style of
tests/point_collect_checks.py, whose collection loop (tables_of), policy (policy_actions), inputs (rollout_checks.make_thetas), replay
(forward32) and bound rule are used as they are.

`norm_update` restates one update of the wrapper's moments in float64 NumPy; `replay_calls` drives it through a recorded sequence of
reset() / step() calls and is pinned by tests/golden/point_env_norm_{corner,momentum,goal}.npz, outputs of the reference's wrapper
(tools/gen_point_norm_golden.py).  `norm_collect_oracle` is the reference's sampler loop of point_collect_checks.collect_oracle with
the wrapper's events in it, for every kind (module docstring of promp_kernels_rollout.h, include/promp_hip.h (b''')):
  reset at the call's start, obs update -> normalised observation -> policy -> raw step -> obs update with the raw next observation
  -> reward update, normalised reward -> if the episode ends, reset at once from start[s + 1] and obs update -- also at the stop step.

The checks run BY INDUCTION FROM WHAT THE DEVICE STORED.  The moments of an environment depend on every step it took up to the stop
step s*, also on the steps of an episode that was still running at s* and whose rows the slab drops.  So every call is issued twice
on the same inputs and the same state: first as a PROBE with a larger total_samples, whose stop step lies where every environment has
finished the episode it was in at s* -- the device's trajectory does not depend on total_samples, so the probe's slab holds the
stored float32 action of every (step <= s*, environment) --, then, with the state put back by promp_point_norm_set, as the call
under test.  (The probe's total_samples is read off the float32 replay on the CPU.)
  * STATES.  The raw float64 states replay exactly from `start` and the stored actions (the stored float32 action is what the device's
    environment consumed), and with them `done`, end_len and the tables: exact equality.
  * MOMENTS.  The replay against promp_point_norm_get after the call: at most 8 * 2^-52 * n_updates * max(1, max x^2), n_updates the
    largest number of updates any environment took in the call (at most 8 roundings per update, the recursion contracts by
    1 - alpha).  Bitwise equality is expected and printed.
  * SLAB.  obs against float32 of the replay's normalised value at ATOL * max(1, |y|), rewards likewise; mean[t] against the oracle
    network at the stored obs[t], act[t] against that mean + exp(log_std) * noise, both by the existing bound rule.
Each case asserts, on the replay's trajectory alone, the events it exists for (events_of): an episode ends at s*, another environment
is in the middle of one (a dropped tail), s* < max_steps - 1, an episode of length 1; every `done` comparison keeps MARGIN from a tie;
every variance that divides stays >= MIN_VAR, so the division amplifies by at most 10.  The fixed-horizon kinds (corner, walls,
momentum) end every episode at the same step: a dropped tail and a length-1 episode cannot occur there and are not asked for;
s* < max_steps - 1 is asked of the fixed-horizon case that stages more steps than total_samples needs (S).  data_seed is chosen on the CPU (test_point_norm_host.py runs the float32 replay of every case).  Nothing is masked.
Each case starts from a non-default state (means in +-0.5, variances in [0.5, 2], different per environment) and runs two
consecutive calls on one context, on steps `step` and 1 - `step`.
"""
import os

import numpy as np

from oracle import point_rollout as pr
from oracle import policy as op
from promp_amd import _lib
from tests import helpers, point_collect_checks as pc, point_family_checks as fc, rollout_checks as rc
from tests.point_collect_checks import collect_oracle, tables_of  # noqa: F401  (the plain loop, used by the flags-off checks)
from tests.rollout_checks import ATOL, ATOL_DEVICE_NOISE, ATOL_LOG_STD, MIN_STD, SEED31, SEED64, bound, maxdev

MARGIN = pc.MARGIN
MIN_VAR = 0.01
EPS = 2.0 ** -52
GOAL_EVENTS = ('ends_at_stop', 'dropped_tail', 'stop_early', 'length_1')
FIXED_EVENTS = ('ends_at_stop',)
STATE_DIM = dict(corner=2, walls=2, momentum=4, goal=2)
TASK_DIM = dict(corner=2, walls=6, momentum=2, goal=2)
MAX_STEP = dict(corner=0.2, walls=0.2, momentum=0.1, goal=0.1)


# ---- the wrapper, float64 -------------------------------------------------------------------------------------------------------

def norm_update(mean, var, x, alpha):
    """one sample (envs/normalized_env.py:73-81): -> (mean', var'), the variance around the NEW mean"""
    mean, var, x = np.asarray(mean, np.float64), np.asarray(var, np.float64), np.asarray(x, np.float64)
    m = (1 - alpha) * mean + alpha * x
    return m, (1 - alpha) * var + alpha * np.square(x - m)


def norm_apply(x, mean, var):
    return (x - mean) / (np.sqrt(var) + 1e-8)


def kind_step(kind, state, action, tasks, env):
    """one raw step for a batch of environments of any kind: state [n, O], action [n, 2] (policy scale), tasks [n, task_dim] ->
    (next state, reward [n], done [n], margin [n]: the distance of the closest evaluated comparison from a tie)"""
    n = len(state)
    if kind == 'goal':
        return pc.goal_step(state, action, tasks, env['normalization_scale'], env['max_step'], env['done_radius'])
    if kind == 'corner':
        assert env['reward_type'] != 'sparse'           # (its equality test between distances is point_rollout's business)
        nxt, rew = pr.env_step(state, action, tasks, **env)
        return nxt, rew, np.zeros(n, bool), np.full(n, np.inf)
    nxt, rew, margin = np.zeros_like(np.asarray(state, np.float64)), np.zeros(n), np.zeros(n)
    for task in np.unique(tasks, axis=0):
        sel = (tasks == task).all(axis=1)
        nxt[sel], rew[sel], info = fc.env_step(kind, state[sel], action[sel], task, **env)
        margin[sel] = info['margin']
    return nxt, rew, np.zeros(n, bool), margin


def load_fixture(name):
    return np.load(os.path.join(helpers.GOLDEN, 'point_env_norm_%s.npz' % name))


FIXTURE_ENV = dict(corner=dict(reward_type='dense', sparse_radius=0.5), momentum=dict(reward_type='dense_squared', sparse_radius=2.0),
                   goal=dict(done_radius=0.01))


def fixture_env(name, g):
    return dict(FIXTURE_ENV[name], normalization_scale=float(g['normalization_scale']), max_step=float(g['action_high'][0]))


def replay_calls(name, g, flags):
    """the fixture's call sequence through norm_update / kind_step -> dict(observations, rewards, dones, obs_mean, obs_var,
    reward_mean, reward_var) as the fixture records them for one flag combination"""
    n_obs, n_rew = bool(flags[0]), bool(flags[1])
    env, O, n = fixture_env(name, g), g['reset_states'].shape[1], len(g['is_reset'])
    oa, ra = float(g['obs_alpha']), float(g['reward_alpha'])
    om, ov, rm, rv = np.zeros(O), np.ones(O), np.float64(0), np.float64(1)
    out = dict(observations=np.zeros((n, O)), rewards=np.zeros(n), dones=np.zeros(n, bool), obs_mean=np.zeros((n, O)),
               obs_var=np.zeros((n, O)), reward_mean=np.zeros(n), reward_var=np.zeros(n))
    state = None
    for c in range(n):
        if g['is_reset'][c]:
            state = g['reset_states'][c].copy()
        else:
            nxt, r, d, _ = kind_step(name, state[None, :], g['actions'][c][None, :], g['task'][None, :], env)
            state, r = nxt[0], r[0]
            if n_rew:
                rm, rv = norm_update(rm, rv, r, ra)
                r = r / (np.sqrt(rv) + 1e-8)
            out['rewards'][c], out['dones'][c] = r, d[0]
        if n_obs:
            om, ov = norm_update(om, ov, state, oa)
        out['observations'][c] = norm_apply(state, om, ov) if n_obs else state
        out['obs_mean'][c], out['obs_var'][c], out['reward_mean'][c], out['reward_var'][c] = om, ov, rm, rv
    return out


# ---- the collection oracle --------------------------------------------------------------------------------------------------------

def split_moments(moments, O):
    m = np.asarray(moments, np.float64)
    return m[:, :O].copy(), m[:, O:2 * O].copy(), m[:, 2 * O].copy(), m[:, 2 * O + 1].copy()


def join_moments(om, ov, rm, rv):
    return np.concatenate([om, ov, rm[:, None], rv[:, None]], axis=1)


def norm_collect_oracle(c, moments, norm, acts=None, known=None, total=None):
    """The sampler loop under the wrapper.  c: a case (norm_case); moments [N, 2 O + 2] the state at entry; norm: dict(normalize_obs,
    normalize_reward, obs_alpha, reward_alpha).  The policy is the float32 replay (forward32, one fmaf for the action) except where
    `known` [S, N] says that acts [S, N, 2] holds the device's stored action.  Runs all S steps, as the device does -> dict(y: the
    normalised observations float64, obs: float32(y), mean, act, rew: the normalised rewards float64, raw: the raw states at every
    step's start, end_len, moments [S, N, W] behind every step, tables, after: moments[stop], margin / min_var / max_x2 /
    n_updates up to the stop step)"""
    kind, spec, th, B, T = c['kind'], c['spec'], c['th'], c['B'], c['T']
    start, z = np.asarray(c['start'], np.float64), c['z']
    S, N, O, M = len(z), start.shape[1], start.shape[2], len(th)
    assert start.shape[0] == S + 1
    n_obs, n_rew = bool(norm['normalize_obs']), bool(norm['normalize_reward'])
    oa, ra = float(norm['obs_alpha']), float(norm['reward_alpha'])
    tasks = np.repeat(np.asarray(c['tasks'], np.float64), B, axis=0)
    om, ov, rm, rv = split_moments(moments, O)
    y, obs, raw = np.zeros((S, N, O)), np.zeros((S, N, O), np.float32), np.zeros((S, N, O))
    mean, act = np.zeros((S, N, 2), np.float32), np.zeros((S, N, 2), np.float32)
    rew, end_len, margins = np.zeros((S, N)), np.zeros((S, N), np.int32), np.zeros((S, N))
    mom, min_var, max_x2, n_upd = np.zeros((S, N, 2 * O + 2)), np.zeros(S), np.zeros(S), np.zeros((S, N), np.int64)
    state, length, count = start[0].copy(), np.zeros(N, np.int64), np.zeros(N, np.int64)
    x2 = 0.0
    if n_obs:
        om, ov = norm_update(om, ov, state, oa)
        count += 1
        x2 = float(np.max(state ** 2))
    for s in range(S):
        raw[s] = state
        y[s] = norm_apply(state, om, ov) if n_obs else state
        obs[s] = y[s].astype(np.float32)
        low = float(ov.min()) if n_obs else np.inf
        mean[s], act[s] = pc.policy_actions(spec, th, obs[s], z[s], B, f32=True)
        if acts is not None:
            act[s] = np.where(known[s][:, None], acts[s], act[s])
        nxt, r, done, margins[s] = kind_step(kind, state, act[s].astype(np.float64), tasks, c['env'])
        length += 1
        end = done | (length >= T)
        end_len[s] = np.where(end, length, 0)
        length[end] = 0
        if n_obs:
            om, ov = norm_update(om, ov, nxt, oa)
            x2 = max(x2, float(np.max(nxt ** 2)))
        if n_rew:
            rm, rv = norm_update(rm, rv, r, ra)
            x2 = max(x2, float(np.max(r ** 2)))
            low = min(low, float(rv.min()))
            r = r / (np.sqrt(rv) + 1e-8)
        rew[s] = r
        count += 1
        state = np.where(end[:, None], start[s + 1], nxt)
        if n_obs and end.any():
            om2, ov2 = norm_update(om, ov, state, oa)
            om, ov = np.where(end[:, None], om2, om), np.where(end[:, None], ov2, ov)
            count += end
            x2 = max(x2, float(np.max(state[end] ** 2)))
        mom[s], min_var[s], max_x2[s], n_upd[s] = join_moments(om, ov, rm, rv), low, x2, count
    tables = tables_of(end_len, M, B, c['total'] if total is None else total)
    out = dict(y=y, obs=obs, mean=mean, act=act, rew=rew, raw=raw, end_len=end_len, moments=mom, tables=tables)
    if tables is not None:
        stop = tables['stop']
        out.update(after=mom[stop], margin=float(margins[:stop + 1].min()), min_var=float(min_var[:stop + 1].min()),
                   max_x2=float(max_x2[stop]), n_updates=int(n_upd[stop].max()))
    return out


def events_of(o, S):
    t, found = o['tables'], {'ends_at_stop'}
    if (o['end_len'][t['stop']] == 0).any():
        found.add('dropped_tail')
    if t['stop'] < S - 1:
        found.add('stop_early')
    if (t['len'] == 1).any():
        found.add('length_1')
    return found


def probe_total(o, T):
    """total_samples of the probe call, on the float32 replay o: its stop step is the first step >= s* by which every environment has
    finished the episode it was in at s*"""
    stop, ends = o['tables']['stop'], o['end_len'] > 0
    later = [int(np.flatnonzero(ends[stop:, e])[0]) for e in range(ends.shape[1])]       # (IndexError: S too small for the probe)
    s_probe = stop + max(later)
    cum = np.cumsum(o['end_len'].sum(axis=1))
    assert s_probe == stop or cum[s_probe] > cum[s_probe - 1]
    return int(cum[s_probe]), s_probe


# ---- cases ------------------------------------------------------------------------------------------------------------------------

def norm_case(kind, M, B, T, hidden, normalization_scale, noise, step, seed, data_seed=0, rollouts=None, S=None, call=0,
              reward_type='dense'):
    """inputs of one call (call 0 / 1 of a case draw different data).  goal: point_collect_checks.goal_case's inputs (starts within
    +-0.05, one step about the box's half-width); S defaults to the sampler's bound plus T, the room the probe needs.  The
    fixed-horizon kinds: S = T * rollouts / B, reset() states of the classes."""
    prng = np.random.RandomState(9000 + 17 * data_seed)            # the policy and the tasks: the same in both calls
    rng = np.random.RandomState(9100 + 17 * data_seed + call)      # start states and noise
    O = STATE_DIM[kind]
    spec = op.PolicySpec(O, 2, hidden, min_std=MIN_STD)
    th = rc.make_thetas(prng, M, O, 2, hidden)
    N, total = M * B, M * (rollouts or B) * T
    env = dict(normalization_scale=float(normalization_scale), max_step=MAX_STEP[kind])
    if kind == 'goal':
        unit = MAX_STEP[kind] / normalization_scale
        th[:, -2:] = (np.log(0.008 / unit) + prng.uniform(-0.3, 0.3, size=(M, 2))).astype(np.float32)
        for i in range(M):                   # one entry of every task below log(MIN_STD): the clip modes differ
            th[i, -2 + i % 2] = np.float32(np.log(MIN_STD) - 0.1 - 0.05 * i)
        env['done_radius'] = pc.DONE_RADIUS
        S = S or pc.max_steps_of(M, B, T, total) + T
        tasks = prng.uniform(-2, 2, size=(M, 2))
        start = rng.uniform(-0.05, 0.05, size=(S + 1, N, 2))
    else:
        env.update(reward_type=reward_type, sparse_radius=2.0)
        assert total % (N * T) == 0
        S = S or total // N
        tasks = rc.CORNERS[prng.choice(4, size=M)]
        if kind == 'walls':
            gaps = prng.uniform(-1, 1, size=(M, 2, 2))
            tasks = np.hstack((tasks, gaps[:, 0] / np.linalg.norm(gaps[:, 0], axis=1)[:, None],
                               2 * gaps[:, 1] / np.linalg.norm(gaps[:, 1], axis=1)[:, None]))
        start = rng.uniform(-0.2, 0.2, size=(S + 1, N, O))
        if kind == 'momentum':
            start[..., 2:] *= 0.5
    if noise == 'host':
        z = rng.randn(S, N, 2).astype(np.float32)
    else:                                    # the staging row is the counter
        z = rc.assert_noise_depends_on_high_word_and_stream(seed, np.arange(S * N), 2, step).reshape(S, N, 2)
    return dict(kind=kind, spec=spec, hidden=hidden, th=th, tasks=tasks, start=start, z=z, env=env, M=M, B=B, T=T, total=total, S=S,
                noise=noise, N=N, O=O)


def initial_moments(N, O, data_seed=0):
    """a wrapper state no fresh wrapper has: means in +-0.5, variances in [0.5, 2], different per environment"""
    rng = np.random.RandomState(400 + data_seed)
    return join_moments(rng.uniform(-0.5, 0.5, size=(N, O)), rng.uniform(0.5, 2.0, size=(N, O)), rng.uniform(-0.5, 0.5, size=N),
                        rng.uniform(0.5, 2.0, size=N))


def case_is_sound(o, c, wanted):
    """the conditions of the module docstring on a replay o"""
    assert o['tables'] is not None, 'the replay does not reach total_samples'
    found = events_of(o, c['S'])
    assert set(wanted) <= found, (sorted(wanted), sorted(found))
    assert o['margin'] >= MARGIN, o['margin']
    assert o['min_var'] >= MIN_VAR, o['min_var']


def wanted_events(c):
    """goal: all four.  A fixed-horizon kind ends every episode at one step; with more staged steps than total_samples needs, the stop
    step lies before the last one and the steps behind it must leave no trace"""
    if c['kind'] == 'goal':
        return GOAL_EVENTS
    return FIXED_EVENTS + (('stop_early',) if c['S'] > c['total'] // c['N'] else ())


def cpu_replay(c, moments, norm):
    """CPU only: the float32 replay of a call, its conditions, the probe's total_samples -> (replay, total, probe step)"""
    o = norm_collect_oracle(c, moments, norm)
    case_is_sound(o, c, wanted_events(c))
    total, s_probe = probe_total(o, c['T'])
    assert s_probe <= c['S'] - 1
    return o, total, s_probe


# ---- the device -------------------------------------------------------------------------------------------------------------------

def open_context(lib, c, K=1):
    rows = c['S'] * c['N']
    ctx = _lib.Context(c['M'], c['O'], 2, c['hidden'], K, max_rows=rows, max_paths=rows, lib=lib)
    ctx.set_min_std(MIN_STD)
    ctx.set_theta(c['th'].mean(axis=0))
    ctx.set_task_thetas(c['th'])
    return ctx


def collect_device(ctx, c, step, seed, clip_infos, norm, **over):
    kw = dict(total_samples=c['total'], max_path_length=c['T'], clip_infos=clip_infos, seed=seed, norm=norm, **c['env'])
    kw.update(over)
    start = kw.pop('start', c['start'])
    z = c['z'][:len(start) - (norm is not None)] if c['noise'] == 'host' else None
    return ctx.collect_point_family(step, c['kind'], c['tasks'], start, z, **kw)


def stored_actions(c, tables, slab):
    """the slab's actions back under their staging rows -> (acts [S, N, 2] float32, known [S, N])"""
    acts, known = np.zeros((c['S'], c['N'], 2), np.float32), np.zeros((c['S'], c['N']), bool)
    pro = tables['path_row_offsets']
    for p, (e, s0, n) in enumerate(zip(tables['path_env'], tables['path_start'], tables['path_len'])):
        acts[s0:s0 + n, e] = slab['act'][pro[p]:pro[p + 1]]
        known[s0:s0 + n, e] = True
    return acts, known


def check_slab(c, o, tables, slab, verbose=''):
    """the SLAB check of the module docstring over the listed paths"""
    spec, th, B = c['spec'], c['th'], c['B']
    t = dict(env=tables['path_env'], start=tables['path_start'], len=tables['path_len'])
    want_y, want_r, z = pc.gather(o['y'], t), pc.gather(o['rew'], t), pc.gather(c['z'], t)
    env_of = np.concatenate([np.full(n, e) for e, n in zip(t['env'], t['len'])])
    assert slab['obs'].shape == want_y.shape and slab['rew'].shape == want_r.shape
    err_obs = np.abs(slab['obs'].astype(np.float64) - want_y.astype(np.float32)) / np.maximum(1.0, np.abs(want_y))
    err_rew = np.abs(slab['rew'].astype(np.float64) - want_r.astype(np.float32)) / np.maximum(1.0, np.abs(want_r))
    atol_act = ATOL if c['noise'] == 'host' else ATOL_DEVICE_NOISE
    tol_mean, tol_act, err_mean, err_act = ATOL, atol_act, 0.0, 0.0
    for i in range(c['M']):
        sel = env_of // B == i
        obs = slab['obs'][sel]
        m_ref = op.forward(spec, th[i].astype(np.float64), obs.astype(np.float64), False)[0]
        m32 = rc.forward32(spec, th[i], obs)
        a_ref = m_ref + np.exp(th[i, -2:].astype(np.float64)) * z[sel]
        a32 = helpers.fma32(np.exp(th[i, -2:]).astype(np.float32)[None, :], z[sel], m32)
        tol_mean, tol_act = max(tol_mean, bound(ATOL, maxdev(m32, m_ref))), max(tol_act, bound(atol_act, maxdev(a32, a_ref)))
        err_mean, err_act = max(err_mean, maxdev(slab['old_mean'][sel], m_ref)), max(err_act, maxdev(slab['act'][sel], a_ref))
    print('%s slab: obs %.2e rew %.2e (of %.1e, relative to max(1, |y|)); mean %.2e of %.2e; act %.2e of %.2e; largest |y| %.2f' % (
        verbose, err_obs.max(), err_rew.max(), ATOL, err_mean, tol_mean, err_act, tol_act, np.abs(want_y).max()))
    assert err_obs.max() <= ATOL and err_rew.max() <= ATOL, (err_obs.max(), err_rew.max())
    assert err_mean <= tol_mean and err_act <= tol_act, (err_mean, tol_mean, err_act, tol_act)


def check_call(ctx, c, norm, step, seed, clip_infos, verbose=''):
    """one call of a case on an open context whose state is set: the probe, the call, the three checks -> the state behind it"""
    N, O = c['N'], c['O']
    before = ctx.get_point_norm(N, O)
    _, total_probe, s_probe = cpu_replay(c, before, norm)
    probe = collect_device(ctx, c, step, seed, clip_infos, norm, total_samples=total_probe)
    acts, known = stored_actions(c, probe, ctx.download_step(step))
    ctx.set_point_norm(before)
    got = collect_device(ctx, c, step, seed, clip_infos, norm)
    slab, after = ctx.download_step(step), ctx.get_point_norm(N, O)
    o = norm_collect_oracle(c, before, norm, acts, known)
    case_is_sound(o, c, wanted_events(c))
    want = o['tables']
    assert known[:want['stop'] + 1].all(), 'the probe does not hold every action up to the stop step'
    assert probe['n_steps'] == s_probe + 1 and probe['n_steps'] >= got['n_steps']
    pc.assert_tables(got, want, c['M'])                                                  # STATES: done, end_len, the tables
    tol = 8 * EPS * o['n_updates'] * max(1.0, o['max_x2'])
    dev = float(np.max(np.abs(after - o['after'])))
    print('%s stop %d of %d steps, %d paths, margin %.2e, smallest variance %.3f; moments: deviation %.2e of %.2e (%d updates, max x^2 '
          '%.2f), bitwise %s' % (verbose, want['stop'], c['S'], len(want['len']), o['margin'], o['min_var'], dev, tol, o['n_updates'],
                                 o['max_x2'], np.array_equal(after, o['after'])))
    assert dev <= tol, (dev, tol)
    assert np.any(after != before)
    if not norm['normalize_obs']:
        assert np.array_equal(after[:, :2 * O], before[:, :2 * O])
    if not norm['normalize_reward']:
        assert np.array_equal(after[:, 2 * O:], before[:, 2 * O:])
    check_slab(c, o, got, slab, verbose)
    np.testing.assert_allclose(slab['old_log_std'], rc.reported_log_std(c['th'], 2, clip_infos), rtol=0, atol=ATOL_LOG_STD)
    return after


def check_norm_collect(lib, kind, M, B, T, hidden, normalization_scale, noise, step, seed, clip_infos, flags, data_seed=0,
                       rollouts=None, S=None, reward_type='dense', obs_alpha=0.05, reward_alpha=0.2):
    norm = dict(normalize_obs=bool(flags[0]), normalize_reward=bool(flags[1]), obs_alpha=obs_alpha, reward_alpha=reward_alpha)
    args = (kind, M, B, T, hidden, normalization_scale, noise)
    c0 = norm_case(*args, step, seed, data_seed, rollouts, S, 0, reward_type)
    c1 = norm_case(*args, 1 - step, seed, data_seed, rollouts, S, 1, reward_type)
    ctx = open_context(lib, c0)
    try:
        ctx.set_point_norm(initial_moments(c0['N'], c0['O'], data_seed))
        label = '%s %s %s flags %s scale %g %s' % (kind, (M, B, T), hidden, tuple(flags), normalization_scale, noise)
        check_call(ctx, c0, norm, step, seed, clip_infos, label + ' call 0:')
        check_call(ctx, c1, norm, 1 - step, seed, clip_infos, label + ' call 1:')
    finally:
        ctx.close()


def case_is_sound_on_cpu(kind, M, B, T, hidden, normalization_scale, noise, step, seed, clip_infos, flags, data_seed=0, rollouts=None,
                         S=None, reward_type='dense', obs_alpha=0.05, reward_alpha=0.2):
    """CPU only: both calls of a case on the float32 replay, the second from the state the first leaves"""
    norm = dict(normalize_obs=bool(flags[0]), normalize_reward=bool(flags[1]), obs_alpha=obs_alpha, reward_alpha=reward_alpha)
    args = (kind, M, B, T, hidden, normalization_scale, noise)
    c0 = norm_case(*args, step, seed, data_seed, rollouts, S, 0, reward_type)
    o0 = cpu_replay(c0, initial_moments(c0['N'], c0['O'], data_seed), norm)[0]
    c1 = norm_case(*args, 1 - step, seed, data_seed, rollouts, S, 1, reward_type)
    o1 = cpu_replay(c1, o0['after'], norm)[0]
    return o0, o1


# ---- flags off, refusals ----------------------------------------------------------------------------------------------------------

def check_flags_off_is_the_plain_call(lib, kind, M, B, T, hidden, noise, step, seed, data_seed=0, rollouts=None):
    """both flags 0: tables and slab are promp_collect_point_family's bit for bit (the staging rows are what the slab is gathered
    from), with a start table one row longer, and the state is not touched"""
    c = norm_case(kind, M, B, T, hidden, 10, noise, step, seed, data_seed, rollouts)
    off = dict(normalize_obs=False, normalize_reward=False, obs_alpha=0.1, reward_alpha=0.2)
    ctx = open_context(lib, c)
    try:
        plain = collect_device(ctx, c, step, seed, True, None, start=c['start'][:-1])
        ref = ctx.download_step(step)
        state = initial_moments(c['N'], c['O'])
        ctx.set_point_norm(state)
        got = collect_device(ctx, c, step, seed, True, off)
        slab = ctx.download_step(step)
        assert np.array_equal(ctx.get_point_norm(c['N'], c['O']), state)
        none_set = open_context(lib, c)                       # and it needs no state at all
        try:
            again = collect_device(none_set, c, step, seed, True, off)
        finally:
            none_set.close()
    finally:
        ctx.close()
    for k in ('n_steps', 'task_path_offsets', 'path_row_offsets', 'path_env', 'path_start', 'path_len'):
        assert np.array_equal(got[k], plain[k]) and np.array_equal(again[k], plain[k]), k
    assert len(plain['path_len']) > 0 and np.any(ref['rew'] != 0)
    for k in ('obs', 'act', 'old_mean', 'rew', 'old_log_std'):
        assert slab[k].shape == ref[k].shape and np.array_equal(slab[k], ref[k]), k


def check_refusals(lib):
    """by name; a refused call leaves the state bit for bit as it was"""
    c = norm_case('goal', 2, 3, 6, (32, 32), 10, 'host', 0, 0)
    on = dict(normalize_obs=True, normalize_reward=True, obs_alpha=0.1, reward_alpha=0.2)
    state = initial_moments(c['N'], c['O'])
    o = norm_collect_oracle(c, state, on)
    assert o['tables'] is not None and o['tables']['stop'] >= 1

    def refused(ctx, match, norm=on, **over):
        try:
            collect_device(ctx, c, 0, 0, True, norm, **over)
        except _lib.PrompError as e:
            assert match in str(e), (match, str(e))
        else:
            raise AssertionError('accepted: expected a refusal naming %r' % match)
    ctx = open_context(lib, c)
    try:
        refused(ctx, 'promp_point_norm_set has not been called')
        try:
            ctx.get_point_norm(c['N'], c['O'])
        except _lib.PrompError as e:
            assert 'has not been called' in str(e)
        else:
            raise AssertionError('read a state that was never set')
        ctx.set_point_norm(state[:-1])                        # another n_envs
        refused(ctx, 'was set for 5 environments')
        ctx.set_point_norm(initial_moments(c['N'], 4))        # another state_dim
        refused(ctx, 'of state_dim 4')
        ctx.set_point_norm(state)
        for bad in (-0.1, 1.5, np.nan, np.inf):
            refused(ctx, 'obs_alpha', dict(on, obs_alpha=bad))
            refused(ctx, 'reward_alpha', dict(on, reward_alpha=bad))
        refused(ctx, 'do not reach total_samples', start=c['start'][:o['tables']['stop'] + 1])     # max_steps one short of s*
        refused(ctx, 'do not reach total_samples', total_samples=c['S'] * c['N'] + 1)
        refused(ctx, 'max_path_length', max_path_length=0)
        assert np.array_equal(ctx.get_point_norm(c['N'], c['O']), state), 'a refused call moved the state'
        collect_device(ctx, c, 0, 0, True, on)                # and the same call with room is accepted
        assert np.any(ctx.get_point_norm(c['N'], c['O']) != state)
    finally:
        ctx.close()
    for cap in ('max_rows', 'max_paths'):                     # too many rows / paths: refused behind the kernels, the state stays
        small = dict(max_rows=c['S'] * c['N'], max_paths=c['S'] * c['N'])
        small[cap] = (o['tables']['rows'] if cap == 'max_rows' else len(o['tables']['len'])) - 1
        ctx = _lib.Context(c['M'], 2, 2, c['hidden'], 1, lib=lib, **small)
        try:
            ctx.set_min_std(MIN_STD)
            ctx.set_task_thetas(c['th'])
            ctx.set_point_norm(state)
            refused(ctx, cap)
            assert np.array_equal(ctx.get_point_norm(c['N'], c['O']), state)
        finally:
            ctx.close()


# ---- the sampler ------------------------------------------------------------------------------------------------------------------

def run_sampler_scenario(name, M=3, B=3, R=4, T=10, hidden=(32, 32), obs_alpha=0.1, reward_alpha=0.2):
    """DevicePointEnvSampler on normalize(MetaPointEnvV2 ('goal') / MetaPointEnvMomentum ('momentum'), normalize_obs=True,
    normalize_reward=True): four obtain_samples calls with host noise, the sampler's draws replayed -- two with a process_samples
    between them, one behind a forced re-creation of the context, one behind set_normalization_state.  Per call: the paths are the
    slab's rows in MetaSampler's order and pass check_slab; the moments against the replay from the state in front of the call, by
    the bound of check_call for every environment.  The actions of episodes that were still running at the stop step are not in
    the sampler's slab: the probe of check_call recovers them, on a context of the test's own with the policy's parameters, the
    replayed inputs (T more staged steps, so that every such episode ends) and the state in front of the call; where the sampler
    stored an action, the probe's must be the same bits.  The caller has bound the library (promp_amd._lib.set_library_for_testing)."""
    from promp_amd.baselines.linear_baseline import LinearFeatureBaseline
    from promp_amd.envs import point_env
    from promp_amd.envs.normalized_env import normalize
    from promp_amd.policies.meta_gaussian_mlp_policy import MetaGaussianMLPPolicy
    from promp_amd.samplers.device_point_sampler import DevicePointEnvSampler
    from promp_amd.samplers.meta_sample_processor import MetaSampleProcessor
    np.random.seed(31)
    O = STATE_DIM[name]
    bare = point_env.MetaPointEnvV2() if name == 'goal' else point_env.MetaPointEnvMomentum(reward_type='dense')
    env = normalize(bare, normalize_obs=True, normalize_reward=True, obs_alpha=obs_alpha, reward_alpha=reward_alpha)
    norm = dict(normalize_obs=True, normalize_reward=True, obs_alpha=obs_alpha, reward_alpha=reward_alpha)
    policy = MetaGaussianMLPPolicy(name='p', obs_dim=O, action_dim=2, meta_batch_size=M, hidden_sizes=hidden)
    sampler = DevicePointEnvSampler(env=env, policy=policy, rollouts_per_meta_task=R, meta_batch_size=M, max_path_length=T,
                                    envs_per_task=B)
    if name == 'momentum':
        B = R                                                 # fixed horizon: one environment per rollout
    N = M * B
    assert sampler.kind == name and sampler.envs_per_task == B
    fresh = sampler.get_normalization_state()
    assert fresh['obs_mean'].shape == (N, O) and not fresh['obs_mean'].any() and (fresh['obs_var'] == 1).all()
    assert fresh['reward_mean'].shape == (N,) and (fresh['reward_var'] == 1).all()
    spec = op.PolicySpec(O, 2, hidden)
    theta = spec.from_ordered_dict(policy.get_param_values())
    theta[-2:] = np.log(0.8)
    policy.set_params(spec.to_ordered_dict(theta))
    policy.switch_to_pre_update()
    proc = MetaSampleProcessor(baseline=LinearFeatureBaseline(), discount=0.99, gae_lambda=1, normalize_adv=True)
    sess = policy.session
    total = M * R * T
    S = T if name == 'momentum' else pc.max_steps_of(M, B, T, total)
    env_opts = dict(normalization_scale=10.0, max_step=MAX_STEP[name])
    env_opts.update(dict(done_radius=0.01) if name == 'goal' else dict(reward_type='dense', sparse_radius=2.0))

    def state_rows(d):
        return join_moments(d['obs_mean'], d['obs_var'], d['reward_mean'], d['reward_var'])

    def one_call(label):
        before = state_rows(sampler.get_normalization_state())
        sampler.update_tasks()
        rng_state = np.random.get_state()
        paths = sampler.obtain_samples()
        np.random.set_state(rng_state)                        # replay the sampler's draws
        if name == 'goal':
            start = np.zeros((S + 1, N, 2))
        else:
            start = np.random.uniform(-0.2, 0.2, size=(S + 1, N, 2))
            start = np.concatenate((start, np.random.uniform(-0.1, 0.1, size=(S + 1, N, 2))), axis=-1)
        z = np.random.normal(size=(S, N, 2)).astype(np.float32)
        fl = paths.flat
        tpo, pro = fl['task_path_offsets'], fl['path_row_offsets']
        lens = np.diff(pro).astype(np.int32)
        p_env = fl.get('path_env', np.arange(N, dtype=np.int32))
        p_start = fl.get('path_start', np.zeros(N, np.int32))
        tables = dict(path_env=p_env, path_start=p_start, path_len=lens, path_row_offsets=pro)
        c = dict(kind=name, spec=spec, hidden=hidden, th=np.tile(theta.astype(np.float32), (M, 1)), tasks=sampler.goals, start=start, z=z,
                 env=env_opts, M=M, B=B, T=T, total=total, S=S, noise='host', N=N, O=O)
        after = state_rows(sampler.get_normalization_state())
        assert np.array_equal(after, sess.ctx.get_point_norm(N, O))
        # the probe: T more staged steps (MetaPointEnvV2 resets to the origin, momentum never has a running episode at its stop step)
        extra = np.random.RandomState(5).randn(T, N, 2).astype(np.float32)
        more = np.zeros((T, N, O)) if name == 'goal' else np.random.RandomState(6).uniform(-0.1, 0.1, size=(T, N, O))
        c = dict(c, S=S + T, start=np.concatenate([start, more]), z=np.concatenate([z, extra]))
        own = stored_actions(c, tables, dict(act=fl['act']))
        total_probe, s_probe = probe_total(norm_collect_oracle(c, before, norm, *own), T)
        ctx = open_context(None, c)
        try:
            ctx.set_min_std(sess.min_std)
            ctx.set_point_norm(before)
            probe = collect_device(ctx, c, 0, 0, True, norm, total_samples=total_probe)
            acts, known = stored_actions(c, probe, ctx.download_step(0))
        finally:
            ctx.close()
        own_acts, own_known = own
        assert (known | ~own_known).all() and np.array_equal(acts[own_known], own_acts[own_known]), 'the probe did not repeat the sampler\'s collection'
        o = norm_collect_oracle(c, before, norm, acts, known)
        t = o['tables']
        assert known[:t['stop'] + 1].all() and probe['n_steps'] == s_probe + 1
        # the tables and the paths, as MetaSampler hands them out: per task, by the step an episode ends at, then by environment
        assert np.array_equal(tpo, t['tpo']) and np.array_equal(p_env, t['env']) and np.array_equal(p_start, t['start']) and \
            np.array_equal(lens, t['len'])
        assert list(paths.keys()) == list(range(M)) and [len(paths[i]) for i in range(M)] == np.diff(tpo).tolist()
        p = 0
        for i in range(M):
            for path in paths[i]:
                rows = slice(pro[p], pro[p + 1])
                for key, arr in (('observations', fl['obs']), ('actions', fl['act']), ('rewards', fl['rew'])):
                    assert np.array_equal(path[key], arr[rows]), key
                assert np.array_equal(path['agent_infos']['mean'], fl['old_mean'][rows]) and path['env_infos'] == {}
                assert np.array_equal(path['agent_infos']['log_std'], np.tile(fl['old_log_std'][i], (lens[p], 1)))
                p += 1
        check_slab(c, o, tables, dict(obs=fl['obs'], act=fl['act'], rew=fl['rew'], old_mean=fl['old_mean']), label)
        # the moments: every environment by the bound of check_call
        tol = 8 * EPS * o['n_updates'] * max(1.0, o['max_x2'])
        dev = float(np.max(np.abs(after - o['after'])))
        tails = int((o['end_len'][t['stop']] == 0).sum())
        print('%s stop %d, %d paths, %d of %d environments with a dropped tail: deviation %.2e of %.2e (bitwise %s)' % (
            label, t['stop'], len(lens), tails, N, dev, tol, np.array_equal(after, o['after'])))
        assert dev <= tol, (dev, tol)
        assert np.any(after != before)
        return paths, before, after

    paths, before, after = one_call('%s sampler call 0:' % name)
    assert np.array_equal(before, state_rows(fresh))
    counter = sess._upload_counter
    sd = proc.process_samples(paths)                          # stays resident
    assert sess._upload_counter == counter and len(sd) == M and sess.resident_slot(sd) is not None
    _, before1, after1 = one_call('%s sampler call 1:' % name)
    assert np.array_equal(before1, after)                     # the state persists across sampling steps
    # a context somebody re-creates is handed the state again
    old = sess.ctx
    sess.ensure(4 * sess.capacity[0], 4 * sess.capacity[1])
    assert sess.ctx is not old
    _, before2, after2 = one_call('%s sampler call 2 (new context):' % name)
    assert np.array_equal(before2, after1)
    # get / set round trip
    got = sampler.get_normalization_state()
    sampler.set_normalization_state(got)
    assert all(np.array_equal(got[k], v) for k, v in sampler.get_normalization_state().items())
    mine = initial_moments(N, O, 3)
    sampler.set_normalization_state(dict(obs_mean=mine[:, :O], obs_var=mine[:, O:2 * O], reward_mean=mine[:, 2 * O], reward_var=mine[:, 2 * O + 1]))
    _, before3, _ = one_call('%s sampler call 3 (state set by hand):' % name)
    assert np.array_equal(before3, mine)
