"""The point-mass family on the device (promp_rollout_point_family: corner, walls, momentum), shared by test_point_family_host.py
(CPU), test_emu_point_family.py (emulator, tiny) and test_gpu_point_family.py (MI355X).  Through the C ABI, in the style of
tests/rollout_checks.py, whose inputs (make_thetas: every task samples under its own parameters, task 0 explores with
log_std = log 12 so that its actions pass the wrapper's box), replay (forward32) and bound rule are used as they are.

`env_step` restates the two environments in float64 NumPy; it is pinned by tests/golden/point_env_{walls,momentum}_*.npz, outputs of
the reference's classes (tools/gen_point_family_golden.py).

Momentum is continuous in every reward type: a free-running float64 oracle (`rollout`), bounds by the existing rule,
max(existing atol, 4 x the deviation of the float32 replay `rollout32` from the oracle), computed on the CPU; a bound above SANITY
is refused; the kernel's output never enters a bound.

Walls is discontinuous (a wall throws the point back by up to 0.28), so no free-running comparison can hold it: a policy output
that differs in its last bit moves a point that grazes a wall to the other side of the comparison.  It is checked by INDUCTION ON
THE SLAB instead: obs[t] against float32(state_t) at ATOL; mean[t] against the oracle network at the stored obs[t], by the bound
rule; act[t] against that mean + exp(log_std) * noise, by the bound rule over ATOL (host noise) or ATOL_DEVICE_NOISE -- task 0's
actions reach magnitude 48, where float32 itself rounds by 1.9e-6, as rollout_checks.py explains for the corner environment --;
then (state_{t+1}, rew[t]) = env_step(state_t, act[t] AS STORED) in float64, the reward at ATOL.  The stored float32 action is
exactly what the device's environment consumed, so the oracle's float64 state follows the device's to rounding and no wall flips,
PROVIDED no comparison is a near tie.  Conditions, asserted on the oracle's trajectory alone, no row masked, no case skipped:
every comparison actually evaluated (|p| and |s'| against 1 or 2, |s' - gap| against 1, and the sparse reward's |s' - goal|
against its radius) has margin >= 1e-9 -- a projected p has norm 1 - ~1e-6 or 2 - ~2e-6 and passes this too --; |reward| < 32 (one
float32 rounding fits ATOL); and the event codes the case is built for all occur: 1 (thrown back at wall 1) and 2 (passed through
its gap) for starts at radius 0.93, 3 and 4 at radius 1.93, half of the starts within 0.3 rad of the gap.  data_seed is chosen so
that this holds.
"""
import os

import numpy as np

from oracle import policy as op, promp as pm
from promp_amd import _lib
from tests import helpers, rollout_checks as rc
from tests.parity_checks import rel_max
from tests.rollout_checks import ATOL, ATOL_DEVICE_NOISE, ATOL_LOG_STD, MIN_STD, SEED31, SEED64, bound, maxdev

KINDS = ('walls', 'momentum')
REWARDS = ('dense', 'dense_squared', 'sparse')
MAX_STEP = dict(corner=0.2, walls=0.2, momentum=0.1)
STATE_DIM = dict(corner=2, walls=2, momentum=4)
MARGIN = 1e-9


# ---- the environments, float64 -------------------------------------------------------------------------------------------------

def _norm(v):
    return np.sqrt(np.sum(v * v, axis=-1))          # squares, sum, root


def _move(action, normalization_scale, max_step):
    action = np.asarray(action, dtype=np.float64)
    lb, ub, s = -max_step, max_step, normalization_scale
    scaled = lb + (action + s) * (ub - lb) / (2 * s) if s > 0 else action
    return np.clip(np.clip(scaled, lb, ub), -max_step, max_step)


def env_step(kind, state, action, task, reward_type, normalization_scale, max_step, sparse_radius):
    """one step for a batch: state [B, state_dim], action [B, 2] (policy scale), task [task_dim] ->
    (next state, reward [B], info): info['event'] [B] the wall event (0 none, 1 wall 1 threw the point back, 2 wall 1 passed through
    the gap, 3 / 4 the same at wall 2), info['margin'] [B] the smallest distance of an evaluated comparison from a tie"""
    state = np.asarray(state, dtype=np.float64)
    task = np.asarray(task, dtype=np.float64)
    move = _move(action, normalization_scale, max_step)
    goal = task[:2]
    B = state.shape[0]
    margin = np.full(B, np.inf)

    def reward(dist, progress_from):
        if reward_type == 'dense':
            return -dist
        if reward_type == 'dense_squared':
            return -dist ** 2
        assert reward_type == 'sparse'
        if kind == 'momentum':
            return np.maximum(sparse_radius - dist, 0.0)
        margin[:] = np.minimum(margin, np.abs(dist - sparse_radius))
        return np.where(dist < sparse_radius, _norm(progress_from - goal) - dist, 0.0)      # (the reference: None outside)

    if kind == 'momentum':
        vel = state[:, 2:] + move
        pos = state[:, :2] + vel
        return np.hstack((pos, vel)), reward(_norm(pos - goal), None), dict(event=np.zeros(B, np.int32), margin=margin)
    assert kind == 'walls'
    nxt = state + move
    rew = reward(_norm(nxt - goal), state)
    before, after = _norm(state), _norm(nxt)
    in1, out1, in2, out2 = before < 1, after > 1, before < 2, after > 2
    first = in1 & out1
    second = ~first & in2 & out2
    far1, far2 = _norm(nxt - task[2:4]) > 1, _norm(nxt - task[4:6]) > 1
    event = np.select([first & far1, first, second & far2, second], [1, 2, 3, 4], 0).astype(np.int32)
    out = nxt.copy()
    out[event == 1] = (nxt / (after + 1e-6)[:, None])[event == 1]
    out[event == 3] = (nxt / (after * 0.5 + 1e-6)[:, None])[event == 3]
    # every comparison in evaluation order: `a and b` stops at a false a, the elif is reached only behind a false first condition
    inf = np.inf
    margin = np.minimum(margin, np.abs(before - 1))
    margin = np.minimum(margin, np.where(in1, np.abs(after - 1), inf))
    margin = np.minimum(margin, np.where(first, np.abs(_norm(nxt - task[2:4]) - 1), inf))
    margin = np.minimum(margin, np.where(~first, np.abs(before - 2), inf))
    margin = np.minimum(margin, np.where(~first & in2, np.abs(after - 2), inf))
    margin = np.minimum(margin, np.where(second, np.abs(_norm(nxt - task[4:6]) - 1), inf))
    return out, rew, dict(event=event, margin=margin)


def load_fixture(kind, reward_type):
    g = np.load(os.path.join(helpers.GOLDEN, 'point_env_%s_%s.npz' % (kind, reward_type)))
    tasks = np.hstack((g['goals'], g['gaps_1'], g['gaps_2'])) if kind == 'walls' else g['goals']
    env = dict(reward_type=reward_type, normalization_scale=float(g['normalization_scale']), max_step=float(g['action_high'][0]),
               sparse_radius=float(g['sparse_reward_radius']))
    return g, tasks, env


def make_env(kind, reward_type, normalization_scale):
    """the package's NumPy class, wrapped as the fixture's was"""
    from promp_amd.envs import point_env
    from promp_amd.envs.normalized_env import normalize
    bare = dict(walls=point_env.MetaPointEnvWalls, momentum=point_env.MetaPointEnvMomentum,
                corner=point_env.MetaPointEnvCorner)[kind](reward_type=reward_type)
    return (normalize(bare, normalization_scale=normalization_scale) if normalization_scale > 0 else bare), bare


def set_env_state(kind, bare, state):
    state = np.asarray(state, dtype=np.float64)
    bare._state = state[:2].copy()
    if kind == 'momentum':
        bare._velocity = state[2:].copy()


def task_of(kind, params):
    params = np.asarray(params, dtype=np.float64)
    return dict(goal=params[:2], gap_1=params[2:4], gap_2=params[4:6]) if kind == 'walls' else params


# ---- rollouts: oracle and float32 replay ----------------------------------------------------------------------------------------

def rollout(kind, spec, th, tasks, start, noise, f32=False, **env):
    """free-running rollout of every task under its own parameters.  f32 False: the float64 oracle (observations handed over as
    float32, the action rounded to float32 in front of the environment, as oracle.point_rollout.rollout); True: the policy as the
    kernels compute it (rollout_checks.forward32, one fmaf for the action, the reward rounded to float32), the environment float64"""
    M, B, T = noise.shape[:3]
    O = STATE_DIM[kind]
    dt = np.float32 if f32 else np.float64
    obs, act, mean, rew = np.zeros((M, B, T, O), dt), np.zeros((M, B, T, 2), dt), np.zeros((M, B, T, 2), dt), np.zeros((M, B, T), dt)
    for i in range(M):
        state = np.asarray(start[i], np.float64).copy()
        sd32 = np.exp(th[i, -2:].astype(np.float32)).astype(np.float32)
        for t in range(T):
            o = state.astype(np.float32)
            if f32:
                m = rc.forward32(spec, th[i], o)
                a = helpers.fma32(sd32[None, :], noise[i, :, t], m)
            else:
                m = op.forward(spec, th[i].astype(np.float64), o.astype(np.float64), False)[0]
                a = m + np.exp(th[i, -2:].astype(np.float64)) * noise[i, :, t]
            obs[i, :, t], mean[i, :, t], act[i, :, t] = o, m, a
            state, r, _ = env_step(kind, state, a.astype(np.float32).astype(np.float64), tasks[i], **env)
            rew[i, :, t] = r
    return dict(obs=obs.reshape(-1, O), act=act.reshape(-1, 2), mean=mean.reshape(-1, 2), rew=rew.reshape(-1))


def make_noise(rng, noise, M, B, T, step, seed):
    if noise == 'host':
        return rng.randn(M, B, T, 2).astype(np.float32)
    return rc.assert_noise_depends_on_high_word_and_stream(seed, np.arange(M * B * T), 2, step).reshape(M, B, T, 2)


def run_device(lib, kind, c, step, seed, clip_infos, noise, hidden_act='tanh', then=None):
    """one promp_rollout_point_family of case c -> the downloaded slab (then(ctx, slab): more work on the open context)"""
    M, B, T = c['z'].shape[:3]
    ctx = _lib.Context(M, STATE_DIM[kind], 2, c['hidden'], 1, max_rows=M * B * T, max_paths=M * B, lib=lib, hidden_act=hidden_act)
    try:
        ctx.set_min_std(MIN_STD)
        ctx.set_theta(c['th'].mean(axis=0))
        ctx.set_task_thetas(c['th'])
        ctx.rollout_point_family(step, kind, c['tasks'], c['start'], noise=c['z'] if noise == 'host' else None,
                                 clip_infos=clip_infos, seed=seed, path_length=T, **c['env'])
        slab = ctx.download_step(step)
        return then(ctx, slab) if then else slab
    finally:
        ctx.close()


# ---- momentum -------------------------------------------------------------------------------------------------------------------

def momentum_case(M, B, T, hidden, reward_type, normalization_scale, noise, step, seed, data_seed=0):
    rng = np.random.RandomState(5000 + data_seed)
    spec = op.PolicySpec(4, 2, hidden, min_std=MIN_STD)
    th = rc.make_thetas(rng, M, 4, 2, hidden, wide_tasks=(0,))
    tasks = rc.CORNERS[rng.choice(4, size=M)]
    start = np.concatenate((rng.uniform(-0.2, 0.2, size=(M, B, 2)), rng.uniform(-0.1, 0.1, size=(M, B, 2))), axis=2)   # reset
    z = make_noise(rng, noise, M, B, T, step, seed)
    env = dict(reward_type=reward_type, normalization_scale=float(normalization_scale), max_step=0.1, sparse_radius=2.0)
    return dict(spec=spec, hidden=hidden, th=th, tasks=tasks, start=start, z=z, env=env)


def check_momentum_rollout(lib, M, B, T, hidden, reward_type, normalization_scale, noise, step, seed, clip_infos=True, data_seed=0):
    c = momentum_case(M, B, T, hidden, reward_type, normalization_scale, noise, step, seed, data_seed)
    spec, th = c['spec'], c['th']
    ref = rollout('momentum', spec, th, c['tasks'], c['start'], c['z'], **c['env'])
    if reward_type == 'sparse':
        assert rc.sparse_guard(ref)
    box = normalization_scale if normalization_scale > 0 else 0.1
    assert (ref['act'] > box).any() and (ref['act'] < -box).any()        # both action-box clips act
    rc.assert_tasks_differ(spec, th, ref['obs'])
    r32 = rollout('momentum', spec, th, c['tasks'], c['start'], c['z'], f32=True, **c['env'])
    dev = {k: maxdev(r32[k], ref[k]) for k in ('obs', 'mean', 'act', 'rew')}
    atol = ATOL if noise == 'host' else ATOL_DEVICE_NOISE
    tol = dict(obs=bound(ATOL, dev['obs']), mean=bound(ATOL, dev['mean']), act=bound(atol, dev['act']), rew=bound(atol, dev['rew']))
    slab = run_device(lib, 'momentum', c, step, seed, clip_infos, noise)
    got = dict(obs=slab['obs'], mean=slab['old_mean'], act=slab['act'], rew=slab['rew'])
    assert got['obs'].shape == (M * B * T, 4)
    err = {k: maxdev(got[k], ref[k]) for k in tol}
    print('momentum %s %s %s scale %g %s step %d: replay deviation %s -> bounds %s; device %s' % (
        (M, B, T), hidden, reward_type, normalization_scale, noise, step, {k: '%.2e' % v for k, v in dev.items()},
        {k: '%.2e' % v for k, v in tol.items()}, {k: '%.2e' % v for k, v in err.items()}))
    for k in ('obs', 'mean', 'act', 'rew'):
        assert err[k] <= tol[k], (k, err[k], tol[k])
    np.testing.assert_allclose(slab['old_log_std'], rc.reported_log_std(th, 2, clip_infos), rtol=0, atol=ATOL_LOG_STD)


def check_momentum_feeds_the_passes(lib, M, B, T, hidden, step, seed, clip_infos):
    """obs_dim 4 reaches the passes: process_samples, one gradient evaluation and one inner_adapt on a momentum slab, against the
    oracle on the DOWNLOADED rows (rollout_checks.check_rollout_feeds_the_passes is the model; the bounds are those of
    parity_checks.check_sample_processing_oracle and check_loss_grad)"""
    from oracle import sample_processing as sp
    c = momentum_case(M, B, T, hidden, 'dense', 10, 'device', step, seed)
    spec, th = c['spec'], c['th']
    alpha = 0.1

    def passes(ctx, slab):
        ctx.process_samples(step, normalize_adv=True)
        proc = ctx.download_processed(step)
        proc = dict(returns=np.array(proc['returns']), advantages=np.array(proc['advantages']))
        g, l, k = ctx.eval_loss_grad(step, 0, clip_log_std=clip_infos)
        ctx.set_step_sizes(np.full(ctx.n_params, alpha, np.float32))
        ctx.inner_adapt(step)
        return slab, proc, g, l, k, ctx.get_task_thetas()
    slab, proc, g, l, k, adapted = run_device(lib, 'momentum', c, step, seed, clip_infos, 'device', then=passes)
    n = B * T
    for i in range(M):
        rows = slice(i * n, (i + 1) * n)
        paths = [dict(observations=slab['obs'][rows][b * T:(b + 1) * T], actions=slab['act'][rows][b * T:(b + 1) * T],
                      rewards=slab['rew'][rows][b * T:(b + 1) * T]) for b in range(B)]
        ref_proc, _ = sp.compute_samples_data(paths, normalize_adv=True)
        np.testing.assert_allclose(proc['returns'][rows], ref_proc['returns'], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(proc['advantages'][rows], ref_proc['advantages'], rtol=1e-4, atol=1e-5)
        sl = dict(observations=slab['obs'][rows], actions=slab['act'][rows], advantages=proc['advantages'][rows],
                  agent_infos=dict(mean=slab['old_mean'][rows], log_std=slab['old_log_std'][i]))
        ref = pm.loss_and_grad(spec, th[i].astype(np.float64), sl, 'ratio', clip_infos)
        np.testing.assert_allclose(l[i], ref['loss'], rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(k[i], ref['kl'], rtol=1e-4, atol=1e-6)
        assert rel_max(g[i], ref['grad']) < 1e-4, i
        raw = pm.loss_and_grad(spec, th[i].astype(np.float64), sl, 'ratio', False)           # the inner step: raw log_std
        assert rel_max(adapted[i].astype(np.float64) - th[i], -alpha * raw['grad']) < 1e-4, i


# ---- walls ----------------------------------------------------------------------------------------------------------------------

WALL_EVENTS = {0.93: (1, 2), 1.93: (3, 4)}


def walls_case(M, B, T, hidden, reward_type, normalization_scale, noise, step, seed, radii, data_seed=0):
    """environment b of a task starts at radius radii[b % len(radii)], at an angle within 0.3 rad of that wall's gap (every other
    one) or 1.3 .. 2 pi - 1.3 rad away from it (where the wall is closed)"""
    rng = np.random.RandomState(6000 + data_seed)
    spec = op.PolicySpec(2, 2, hidden, min_std=MIN_STD)
    th = rc.make_thetas(rng, M, 2, 2, hidden, wide_tasks=(0,))
    goals = rc.CORNERS[rng.choice(4, size=M)]
    g1, g2 = rng.randn(M, 2), rng.randn(M, 2)
    g1 /= np.linalg.norm(g1, axis=1)[:, None]
    g2 /= (np.linalg.norm(g2, axis=1) / 2)[:, None]
    tasks = np.hstack((goals, g1, g2))
    start = np.zeros((M, B, 2))
    for i in range(M):
        for b in range(B):
            r = radii[b % len(radii)]
            gap = g1[i] if r < 1 else g2[i]
            near = (b // len(radii)) % 2 == 0
            ang = np.arctan2(gap[1], gap[0]) + (rng.uniform(-0.3, 0.3) if near else rng.uniform(1.3, 2 * np.pi - 1.3))
            start[i, b] = r * np.array([np.cos(ang), np.sin(ang)])
    z = make_noise(rng, noise, M, B, T, step, seed)
    env = dict(reward_type=reward_type, normalization_scale=float(normalization_scale), max_step=0.2, sparse_radius=2.0)
    return dict(spec=spec, hidden=hidden, th=th, tasks=tasks, start=start, z=z, env=env, radii=radii)


def walls_induction(c, obs, act, rew, mean, verbose=''):
    """the induction of the module docstring over a slab (obs / act / mean [M][B][T][2], rew [M][B][T]) -> the events met"""
    spec, th, z = c['spec'], c['th'], c['z']
    M, B, T = z.shape[:3]
    host = z.dtype == np.float32
    atol_act = ATOL if host else ATOL_DEVICE_NOISE
    rc.assert_tasks_differ(spec, th, obs.reshape(M, -1, 2))
    events, margin, err = set(), np.inf, dict(obs=0.0, mean=0.0, act=0.0, rew=0.0)
    tol_mean, tol_act, rew_max = ATOL, atol_act, 0.0
    for i in range(M):
        state = np.asarray(c['start'][i], np.float64).copy()
        for t in range(T):
            err['obs'] = max(err['obs'], maxdev(obs[i, :, t], state.astype(np.float32)))
            o = obs[i, :, t]
            m_ref = op.forward(spec, th[i].astype(np.float64), o.astype(np.float64), False)[0]
            m32 = rc.forward32(spec, th[i], o)
            a_ref = m_ref + np.exp(th[i, -2:].astype(np.float64)) * z[i, :, t]
            a32 = helpers.fma32(np.exp(th[i, -2:]).astype(np.float32)[None, :], z[i, :, t], m32)
            tol_mean, tol_act = max(tol_mean, bound(ATOL, maxdev(m32, m_ref))), max(tol_act, bound(atol_act, maxdev(a32, a_ref)))
            err['mean'] = max(err['mean'], maxdev(mean[i, :, t], m_ref))
            err['act'] = max(err['act'], maxdev(act[i, :, t], a_ref))
            state, r, info = env_step('walls', state, act[i, :, t].astype(np.float64), c['tasks'][i], **c['env'])
            err['rew'] = max(err['rew'], maxdev(rew[i, :, t], r))
            rew_max = max(rew_max, float(np.max(np.abs(r))))
            events |= set(int(e) for e in info['event'])
            margin = min(margin, float(info['margin'].min()))
    tol = dict(obs=ATOL, mean=tol_mean, act=tol_act, rew=ATOL)
    print('%s events %s margin %.2e |rew| %.3g; bounds %s; device %s' % (
        verbose, sorted(events), margin, rew_max, {k: '%.2e' % v for k, v in tol.items()}, {k: '%.2e' % v for k, v in err.items()}))
    return events, margin, rew_max, err, tol


def assert_walls_conditions(c, events, margin, rew_max, acts):
    """on the oracle's trajectory alone"""
    wanted = set(e for r in c['radii'] for e in WALL_EVENTS[r])
    assert wanted <= events, (sorted(wanted), sorted(events))
    assert margin >= MARGIN, margin
    assert rew_max < 32.0, rew_max
    box = c['env']['normalization_scale'] if c['env']['normalization_scale'] > 0 else 0.2
    assert (acts > box).any() and (acts < -box).any()        # both action-box clips act


def check_walls_rollout(lib, M, B, T, hidden, reward_type, normalization_scale, noise, step, seed, radii, clip_infos=True, data_seed=0):
    c = walls_case(M, B, T, hidden, reward_type, normalization_scale, noise, step, seed, radii, data_seed)
    slab = run_device(lib, 'walls', c, step, seed, clip_infos, noise)
    shape = (M, B, T)
    obs, act, mean, rew = slab['obs'].reshape(shape + (2,)), slab['act'].reshape(shape + (2,)), slab['old_mean'].reshape(shape + (2,)), slab['rew'].reshape(shape)
    events, margin, rew_max, err, tol = walls_induction(c, obs, act, rew, mean, 'walls %s %s %s scale %g %s step %d:' % (
        shape, hidden, reward_type, normalization_scale, noise, step))
    assert_walls_conditions(c, events, margin, rew_max, act)
    if reward_type == 'sparse':
        assert 0 < np.count_nonzero(rew) < rew.size
    for k in ('obs', 'mean', 'act', 'rew'):
        assert err[k] <= tol[k], (k, err[k], tol[k])
    np.testing.assert_allclose(slab['old_log_std'], rc.reported_log_std(c['th'], 2, clip_infos), rtol=0, atol=ATOL_LOG_STD)


def walls_case_is_sound(M, B, T, hidden, reward_type, normalization_scale, noise, step, seed, radii, clip_infos=True, data_seed=0):
    """CPU only: the case's conditions on the float32 replay's free-running trajectory (what data_seed was chosen by)"""
    c = walls_case(M, B, T, hidden, reward_type, normalization_scale, noise, step, seed, radii, data_seed)
    r = rollout('walls', c['spec'], c['th'], c['tasks'], c['start'], c['z'], f32=True, **c['env'])
    shape = (M, B, T)
    events, margin, rew_max, err, tol = walls_induction(c, r['obs'].reshape(shape + (2,)), r['act'].reshape(shape + (2,)),
                                                        r['rew'].reshape(shape), r['mean'].reshape(shape + (2,)))
    assert_walls_conditions(c, events, margin, rew_max, r['act'])
    if reward_type == 'sparse':
        assert 0 < np.count_nonzero(r['rew']) < r['rew'].size
    return margin


# ---- corner through the new entry point, refusals -------------------------------------------------------------------------------

def check_corner_bitwise(lib, M, B, T, hidden, reward_type, normalization_scale, noise, step, seed, clip_infos=True):
    """kind 0 of promp_rollout_point_family == promp_rollout_point_env on the same inputs, bit for bit"""
    c = rc.point_case(M, B, T, hidden, reward_type, normalization_scale, noise, step, seed, clip_infos)
    slabs = []
    for family in (False, True):
        ctx = _lib.Context(M, 2, 2, hidden, 1, max_rows=M * B * T, max_paths=M * B, lib=lib)
        try:
            ctx.set_min_std(MIN_STD)
            ctx.set_theta(c['th'].mean(axis=0))
            ctx.set_task_thetas(c['th'])
            kw = dict(noise=c['z'] if noise == 'host' else None, clip_infos=clip_infos, seed=seed, path_length=T, **c['env'])
            if family:
                ctx.rollout_point_family(step, 'corner', c['goals'], c['start'], **kw)
            else:
                ctx.rollout_point_env(step, c['goals'], c['start'], **kw)
            slabs.append(ctx.download_step(step))
        finally:
            ctx.close()
    assert np.any(slabs[0]['rew'] != 0) and np.all(np.isfinite(slabs[0]['act']))
    for k in ('obs', 'act', 'old_mean', 'rew', 'old_log_std'):
        assert slabs[0][k].shape == slabs[1][k].shape and np.array_equal(slabs[0][k], slabs[1][k]), k


def check_refusals(lib):
    rng = np.random.RandomState(0)
    M, B, T = 2, 2, 2

    def refused(match, O=2, A=2, kind='walls', task_dim=6, state_dim=2, **kw):
        ctx = _lib.Context(M, O, A, (32, 32), 1, max_rows=M * B * T, max_paths=M * B, lib=lib)
        try:
            ctx.rollout_point_family(0, kind, rng.randn(M, task_dim), rng.randn(M, B, state_dim), noise=rng.randn(M, B, T, 2), **kw)
        except _lib.PrompError as e:
            assert match in str(e), (match, str(e))
        else:
            raise AssertionError('accepted: expected a refusal naming %r' % match)
        finally:
            ctx.close()
    refused('unknown environment kind', kind=3)
    refused('unknown environment kind', kind=-1)
    refused('task_dim', kind=1, task_dim=2)                      # walls with a bare goal
    refused('task_dim', kind=2, task_dim=6, state_dim=4, O=4)    # momentum with walls' parameters
    refused('task_dim', kind=0, task_dim=6)
    refused('obs_dim', kind='momentum', task_dim=2, state_dim=4, O=2)
    refused('obs_dim', kind='walls', O=4)
    refused('act_dim', kind='walls', A=3)
