"""The kernels that PRODUCE the training data (k_policy_step / k_gen_policy_step, k_point_rollout / k_gen_point_rollout,
k_gather_paths, k_policy_forward / k_gen_policy_forward), shared by test_emu_rollout.py (emulator, tiny) and test_gpu_rollout.py
(MI355X).  Everything goes through the C ABI (promp_amd._lib.Context): no sampler classes, no np.random replay.

What the scenarios of test_plugin_api.py cannot see and these checks can: every task samples under ITS OWN parameters
(set_task_thetas, th[i] = theta + 0.05 randn, log_std different per task and per action, at least one entry below log(min_std)
with min_std = 0.5); more than one block / loop trip; every two-layer family and the zero-padded widths; the fixed slab layout
of promp_begin_rollout; a 64-bit seed, stream = step 1, act_dim 1 and 8; clip_infos on and off; hand-written path tables.

References (float64): oracle.policy.forward, oracle.point_rollout.rollout (one theta per task), oracle.philox.action_noise at
the layout's own counters (fixed: env * T + t; staged: t * M * B + env; point rollouts: env * T + t), stream = step.

Tolerances.  The scenarios of test_plugin_api.py hold the rollout kernels to atol 2e-6 (observations, means, host-noise actions
and rewards), 5e-6 (actions and rewards with device noise) and 1e-6 (log_std), measured at widths up to 64.  Wider layers, 111
to 376 inputs and actions of magnitude 12 x 4 round more in float32 whatever the kernel does, so every case computes its own
yardstick on the CPU: forward32 / rollout32 below replay the kernels' index-order fmaf sums in NumPy float32
(tests.helpers.fma32), and the case allows max(existing atol, 4 x the replay's largest deviation from the float64 oracle on
the case's own inputs).  The factor 4 covers fast_tanh and the device's expf / logf / cosf / sinf against NumPy's.  The
kernel's output never enters the bound.  A bound above SANITY (2e-5) is refused: it would mean the inputs sit on a
discontinuity of the environment (sparse reward), where the comparison says nothing.

Largest replay deviation from the oracle and the resulting bound, per case of test_gpu_rollout.py.  The policy-step actions keep
5e-6 in every case (replay deviation at most 1.2e-6) and log_std keeps 1e-6; a case or field that is not listed keeps the
existing atol, as does every case of test_emu_rollout.py but those marked (emu):

    policy step (M,B,T,O,A,hidden)              means: deviation -> bound
    (2,64,2,20,6,(64,64))                       5.10e-7 -> 2.04e-6
    (2,130,2,20,8,(64,64))                      5.85e-7 -> 2.34e-6
    (2,5,3,111,8,(128,128))                     6.78e-7 -> 2.71e-6    (emu, B = 2: the same)
    (2,5,3,50,4,(100,100))                      6.35e-7 -> 2.54e-6
    (2,5,3,100,6,(64,64))                       6.12e-7 -> 2.45e-6    (emu, B = 2: 5.83e-7 -> 2.33e-6)
    (2,3,3,376,17,(64,64))                      1.16e-6 -> 4.64e-6    (emu, B = 2: the same)
    (2,3,3,30,6,(256,256)) relu                 5.77e-7 -> 2.31e-6
    (emu) (2,3,2,20,8,(64,64))                  5.55e-7 -> 2.22e-6
    policy forward (M,batch,O,A,hidden)         means: deviation -> bound
    (3,256 / 257,20,6,(64,64))                  1.00e-6 -> 4.02e-6
    (3,513,20,6,(64,64))                        9.94e-7 -> 3.98e-6
    (3,256 / 257,20,6,(64,64,64))               6.17e-7 -> 2.47e-6
    (3,513,20,6,(64,64,64))                     7.01e-7 -> 2.80e-6
    (2,257,111,8,(128,128))                     1.20e-6 -> 4.78e-6
    (2,257,50,4,(100,100))                      7.83e-7 -> 3.13e-6
    point rollout (M,B,T,hidden), noise         actions: deviation -> bound           (observations, means: 2e-6 everywhere)
    (3,65,12,(32,32)) sparse, host              2.59e-6 -> 1.04e-5
    (2,129,8,(64,64)) dense, device             2.54e-6 -> 1.02e-5
    (2,5,40,(128,128)) dense_squared, device    1.96e-6 -> 7.83e-6
    (2,5,20,(100,100)) sparse, host             1.76e-6 -> 7.02e-6
    (2,4,1,(32,32)) dense, device               1.63e-6 -> 6.51e-6
    (3,1,16,(64,64)) dense, host                1.44e-6 -> 5.75e-6
    (2,3,12,(32,16,24)) sparse, device          1.76e-6 -> 7.05e-6
    (2,3,10,(24,24)) linear, dense_squared, host  1.48e-6 -> 5.92e-6; rewards 5.87e-7 -> 2.35e-6
    (emu) (2,65,2,(32,32)) host / device        1.49e-6 -> 5.97e-6 / 1.45e-6 -> 5.82e-6
    (emu) (2,2,2,(100,100)) / (2,2,2,(24,24))   6.80e-7 -> 2.72e-6 / 8.71e-7 -> 3.49e-6

The point-rollout actions are the one place where the existing 2e-6 cannot hold whatever the kernel does: task 0 explores with
log_std = log 12, an action of magnitude 16 .. 64 is rounded to float32 once (half an ulp: 0.95e-6 .. 1.9e-6) and its scale
exp(log 12) once more, and B = 65 .. 129 environments reach those magnitudes where the 12 of the existing scenario do not.
"""
import itertools

import numpy as np

from oracle import philox, point_rollout as pr, policy as op, promp as pm
from promp_amd import _lib, synthetic
from tests import helpers
from tests.parity_checks import rel_max

MIN_STD = 0.5             # a benign floor (check_loss_grad's): values below it stay comparable in float32
ATOL, ATOL_DEVICE_NOISE, ATOL_LOG_STD = 2e-6, 5e-6, 1e-6
SANITY = 2e-5
CORNERS = np.array([[-2.0, -2.0], [2.0, -2.0], [-2.0, 2.0], [2.0, 2.0]])
SEED64 = 0x9E3779B97F4A7C15       # nonzero high and low words
SEED31 = 0x2545F491               # below 2^31


# ---- inputs ---------------------------------------------------------------------------------------------------------------------

def make_thetas(rng, M, O, A, hidden, wide_tasks=()):
    """[M][Theta] float32: th[i] = theta + 0.05 randn; log_std different per task and per action, one entry of every task below
    log(MIN_STD); tasks in wide_tasks get log_std around log 12 (actions beyond the point environment's +-10 box) instead"""
    theta = synthetic.init_theta(rng, O, hidden, A).astype(np.float64)
    th = theta + 0.05 * rng.randn(M, theta.size)
    ls = rng.uniform(-0.6, 0.0, size=(M, A))
    for i in range(M):
        if i in wide_tasks:
            ls[i] = np.log(12.0) + 0.05 * np.arange(A)
        else:
            ls[i, i % A] = np.log(MIN_STD) - 0.2 - 0.1 * i
    th[:, -A:] = ls
    th = th.astype(np.float32)
    assert (th[:, -A:] < np.log(MIN_STD)).any() and len(np.unique(th[:, -A:])) == M * A
    return th


def reported_log_std(th, A, clip_infos):
    """what agent_infos carry: max(log_std, log(min_std)) from the pre-update policy, the raw values otherwise"""
    raw = th[:, -A:].astype(np.float64)
    clipped = np.maximum(raw, np.log(MIN_STD))
    assert np.any(clipped != raw)            # one entry lies below the floor: the two differ
    return clipped if clip_infos else raw


# ---- references -----------------------------------------------------------------------------------------------------------------

def forward32(spec, theta32, obs32):
    """the rollout kernels' mean network in NumPy float32: every unit starts from its bias and adds its inputs in index order,
    one fused multiply-add (one rounding) each -- mlp_mean, k_policy_forward, gen_mlp_block; tanh is NumPy's float32 tanh"""
    parts = spec.unflatten(np.asarray(theta32, np.float32))
    x = np.asarray(obs32, np.float32)
    nl = len(spec.layer_shapes)
    for li in range(nl):
        W, b = parts[2 * li], parts[2 * li + 1]
        z = np.tile(b.astype(np.float32), (x.shape[0], 1))
        for k in range(W.shape[0]):
            z = helpers.fma32(x[:, k:k + 1], W[k:k + 1, :], z)
        kind = spec.hidden_act if li < nl - 1 else spec.output_act
        x = (np.tanh(z) if kind == 'tanh' else np.maximum(z, np.float32(0)) if kind == 'relu' else z).astype(np.float32)
    return x


def task_means(spec, th, obs, f32=False):
    """obs [M][n][O] -> means [M][n][A] under each task's own parameters (float64 oracle, or the float32 replay)"""
    if f32:
        return np.stack([forward32(spec, th[i], obs[i]) for i in range(len(th))])
    return np.stack([op.forward(spec, th[i].astype(np.float64), obs[i].astype(np.float64), False)[0] for i in range(len(th))])


def assert_tasks_differ(spec, th, obs):
    """on the oracle alone: any two tasks' means on the test's observations differ by far more than any tolerance here"""
    allobs = np.asarray(obs, np.float64).reshape(-1, spec.obs_dim)
    means = [op.forward(spec, t.astype(np.float64), allobs, False)[0] for t in th]
    gap = min(np.max(np.abs(a - b)) for a, b in itertools.combinations(means, 2))
    assert gap > 1e-3, gap


def bound(atol, *deviations):
    b = max([atol] + [4.0 * float(d) for d in deviations])
    assert b <= SANITY, (atol, deviations)
    return b


def maxdev(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def assert_noise_depends_on_high_word_and_stream(seed, rows, A, stream):
    """oracle side, same rows: the second key word and the stream are part of the draw"""
    base = philox.action_noise(seed, rows, A, stream)
    hi = philox.action_noise(seed ^ (1 << 32), rows, A, stream)
    st = philox.action_noise(seed, rows, A, stream + 1)
    for other in (hi, st):
        assert np.mean(np.abs(other - base) > 1e-3) > 0.9
    return base


def rollout32(spec, th, goals, start, noise, **env):
    """oracle.point_rollout.rollout with the policy in float32 as the kernels compute it (forward32, one fmaf for the action, the
    reward rounded to float32); the environment stays the oracle's float64 env_step, as on the device"""
    M, B, T = noise.shape[:3]
    obs, act, mean = (np.zeros((M, B, T, 2), np.float32) for _ in range(3))
    rew = np.zeros((M, B, T), np.float32)
    for i in range(M):
        sd = np.exp(th[i, -2:].astype(np.float32)).astype(np.float32)
        state = np.asarray(start[i], np.float64).copy()
        for t in range(T):
            o = state.astype(np.float32)
            m = forward32(spec, th[i], o)
            a = helpers.fma32(sd[None, :], noise[i, :, t], m)
            obs[i, :, t], mean[i, :, t], act[i, :, t] = o, m, a
            state, r = pr.env_step(state, a.astype(np.float64), np.asarray(goals[i], np.float64), **env)
            rew[i, :, t] = r.astype(np.float32)
    return dict(obs=obs.reshape(-1, 2), act=act.reshape(-1, 2), mean=mean.reshape(-1, 2), rew=rew.reshape(-1))


# ---- A: promp_begin_rollout / promp_begin_collection + promp_policy_step -----------------------------------------------------------

def collect(lib, M, B, T, O, A, hidden, layout, step, seed, clip_infos, hidden_act='tanh', output_act=None, data_seed=0):
    """T policy steps on seeded observations into step `step`'s slab, fixed layout or staged with every environment one
    full-length path.  -> dict with the OPEN context (the caller closes it) and everything fed and returned"""
    assert layout in ('fixed', 'staged')
    rng = np.random.RandomState(1000 + data_seed)
    spec = op.PolicySpec(O, A, hidden, min_std=MIN_STD, hidden_act=hidden_act, output_act=output_act or 'identity')
    th = make_thetas(rng, M, O, A, hidden)
    obs = rng.randn(T, M, B, O).astype(np.float32)
    rew = rng.randn(M * B * T).astype(np.float32)
    ctx = _lib.Context(M, O, A, hidden, 1, max_rows=M * B * T, max_paths=M * B, lib=lib, hidden_act=hidden_act, output_act=output_act)
    try:
        ctx.set_min_std(MIN_STD)
        ctx.set_theta(th.mean(axis=0))
        ctx.set_task_thetas(th)
        if layout == 'fixed':
            ctx.begin_rollout(step, B, T)
        else:
            ctx.begin_collection(step, B, T)
        acts = np.stack([ctx.policy_step(step, t, obs[t], seed=seed, clip_infos=clip_infos) for t in range(T)])
        if layout == 'staged':
            ctx.end_collection(step, np.arange(M + 1) * B, np.arange(M * B), np.zeros(M * B), np.full(M * B, T), rew)
        else:
            ctx.set_rewards(step, rew)
        slab = ctx.download_step(step)
    except Exception:
        ctx.close()
        raise
    env, t = np.divmod(np.arange(M * B * T), T)              # slab row = env * T + t in both layouts
    counters = env * T + t if layout == 'fixed' else t * (M * B) + env
    return dict(ctx=ctx, spec=spec, th=th, slab=slab, rew=rew, counters=counters,
                fed=obs.transpose(1, 2, 0, 3).reshape(M * B * T, O), returned=acts.transpose(1, 2, 0, 3).reshape(M * B * T, A))


def assert_policy_rows(spec, th, M, A, obs_rows, act_rows, mean_rows, counters, seed, stream, verbose=''):
    """rows in task order, the same number per task: means against the oracle under each task's theta, actions against
    mean + exp(RAW log_std) * the oracle's Philox noise at `counters`"""
    obs_t = obs_rows.reshape(M, -1, spec.obs_dim)
    assert_tasks_differ(spec, th, obs_t)
    noise = assert_noise_depends_on_high_word_and_stream(seed, counters, A, stream).reshape(M, -1, A)
    mean_ref = task_means(spec, th, obs_t)
    act_ref = mean_ref + np.exp(th[:, None, -A:].astype(np.float64)) * noise
    m32 = task_means(spec, th, obs_t, f32=True)
    a32 = helpers.fma32(np.exp(th[:, None, -A:]).astype(np.float32), noise, m32)
    d_mean, d_act = maxdev(m32, mean_ref), maxdev(a32, act_ref)
    tol_mean, tol_act = bound(ATOL, d_mean), bound(ATOL_DEVICE_NOISE, d_act)
    e_mean, e_act = maxdev(mean_rows.reshape(M, -1, A), mean_ref), maxdev(act_rows.reshape(M, -1, A), act_ref)
    print('%s replay deviation mean %.2e act %.2e -> bounds %.2e %.2e; device mean %.2e act %.2e' % (
        verbose, d_mean, d_act, tol_mean, tol_act, e_mean, e_act))
    assert e_mean <= tol_mean, (e_mean, tol_mean)
    assert e_act <= tol_act, (e_act, tol_act)


def check_policy_step(lib, M, B, T, O, A, hidden, layout, step, seed, clip_infos, hidden_act='tanh', output_act=None):
    r = collect(lib, M, B, T, O, A, hidden, layout, step, seed, clip_infos, hidden_act, output_act)
    r['ctx'].close()
    slab, th = r['slab'], r['th']
    np.testing.assert_array_equal(slab['obs'], r['fed'])
    np.testing.assert_array_equal(slab['act'], r['returned'])
    np.testing.assert_array_equal(slab['rew'], r['rew'])
    assert_policy_rows(r['spec'], th, M, A, slab['obs'], slab['act'], slab['old_mean'], r['counters'], seed, step,
                       'policy_step %s %s %s step %d clip %d:' % ((M, B, T, O, A), hidden, layout, step, clip_infos))
    assert slab['old_log_std'].shape == (M, A)
    np.testing.assert_allclose(slab['old_log_std'], reported_log_std(th, A, clip_infos), rtol=0, atol=ATOL_LOG_STD)


# ---- E: what the rollout wrote is what the passes read -----------------------------------------------------------------------------

def check_rollout_feeds_the_passes(lib, M, B, T, O, A, hidden, step, seed, clip_infos, hidden_act='tanh', output_act=None):
    """after a staged collection: advantages in, one gradient evaluation at the sampling parameters, against the oracle on the
    DOWNLOADED slab -- the compact [M][A] old_ls of the rollout is what the pass kernels read back (check_loss_grad's bounds)"""
    r = collect(lib, M, B, T, O, A, hidden, 'staged', step, seed, clip_infos, hidden_act, output_act)
    ctx, spec, th, slab = r['ctx'], r['spec'], r['th'], r['slab']
    try:
        rng = np.random.RandomState(7)
        ctx.set_rewards(step, rng.randn(M * B * T).astype(np.float32))
        adv = rng.randn(M * B * T).astype(np.float32)
        ctx.set_advantages(step, adv)
        g, l, k = ctx.eval_loss_grad(step, 0, clip_log_std=clip_infos)
    finally:
        ctx.close()
    n = B * T
    for i in range(M):
        rows = slice(i * n, (i + 1) * n)
        sl = dict(observations=slab['obs'][rows], actions=slab['act'][rows], advantages=adv[rows],
                  agent_infos=dict(mean=slab['old_mean'][rows], log_std=slab['old_log_std'][i]))
        ref = pm.loss_and_grad(spec, th[i].astype(np.float64), sl, 'ratio', clip_infos)
        np.testing.assert_allclose(l[i], ref['loss'], rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(k[i], ref['kl'], rtol=1e-4, atol=1e-6)
        assert rel_max(g[i], ref['grad']) < 1e-4, i


# ---- B: promp_rollout_point_env ----------------------------------------------------------------------------------------------------

def point_case(M, B, T, hidden, reward_type, normalization_scale, noise, step, seed, clip_infos=True, hidden_act='tanh', data_seed=0):
    """inputs and float64 reference of one point rollout (CPU only): task 0 explores with log_std = log 12"""
    rng = np.random.RandomState(2000 + data_seed)
    spec = op.PolicySpec(2, 2, hidden, min_std=MIN_STD, hidden_act=hidden_act)
    th = make_thetas(rng, M, 2, 2, hidden, wide_tasks=(0,))
    goals = CORNERS[rng.choice(4, size=M)]
    start = rng.uniform(-0.2, 0.2, size=(M, B, 2))
    if noise == 'host':
        z = rng.randn(M, B, T, 2).astype(np.float32)
    else:
        z = assert_noise_depends_on_high_word_and_stream(seed, np.arange(M * B * T), 2, step).reshape(M, B, T, 2)
    env = dict(reward_type=reward_type, normalization_scale=float(normalization_scale), max_step=0.2, sparse_radius=0.5)
    ref = pr.rollout(spec, th.astype(np.float64), goals, start, z, clip_infos=clip_infos, **env)
    return dict(spec=spec, th=th, goals=goals, start=start, z=z, env=env, ref=ref)


def sparse_guard(ref):
    return 0 < np.count_nonzero(ref['rew']) < ref['rew'].size


def check_point_rollout(lib, M, B, T, hidden, reward_type, normalization_scale, noise, step, seed, clip_infos=True,
                        hidden_act='tanh', data_seed=0):
    c = point_case(M, B, T, hidden, reward_type, normalization_scale, noise, step, seed, clip_infos, hidden_act, data_seed)
    spec, th, ref = c['spec'], c['th'], c['ref']
    if reward_type == 'sparse':
        assert sparse_guard(ref)              # a condition on the inputs
    box = normalization_scale if normalization_scale > 0 else 0.2
    assert (ref['act'] > box).any() and (ref['act'] < -box).any()        # both action-box clips act
    assert_tasks_differ(spec, th, ref['obs'])
    r32 = rollout32(spec, th, c['goals'], c['start'], c['z'], **c['env'])
    dev = {k: maxdev(r32[k], ref[k]) for k in ('obs', 'mean', 'act', 'rew')}
    atol = ATOL if noise == 'host' else ATOL_DEVICE_NOISE
    tol = dict(obs=bound(ATOL, dev['obs']), mean=bound(ATOL, dev['mean']), act=bound(atol, dev['act']), rew=bound(atol, dev['rew']))
    ctx = _lib.Context(M, 2, 2, hidden, 1, max_rows=M * B * T, max_paths=M * B, lib=lib, hidden_act=hidden_act)
    try:
        ctx.set_min_std(MIN_STD)
        ctx.set_theta(th.mean(axis=0))
        ctx.set_task_thetas(th)
        ctx.rollout_point_env(step, c['goals'], c['start'], noise=c['z'] if noise == 'host' else None, clip_infos=clip_infos,
                              seed=seed, path_length=T, **c['env'])
        slab = ctx.download_step(step)
    finally:
        ctx.close()
    got = dict(obs=slab['obs'], mean=slab['old_mean'], act=slab['act'], rew=slab['rew'])
    err = {k: maxdev(got[k], ref[k]) for k in tol}
    print('point_rollout %s %s %s scale %g %s step %d: replay deviation %s -> bounds %s; device %s' % (
        (M, B, T), hidden, reward_type, normalization_scale, noise, step, {k: '%.2e' % v for k, v in dev.items()},
        {k: '%.2e' % v for k, v in tol.items()}, {k: '%.2e' % v for k, v in err.items()}))
    for k in ('obs', 'mean', 'act', 'rew'):
        assert err[k] <= tol[k], (k, err[k], tol[k])
    np.testing.assert_allclose(slab['old_log_std'], reported_log_std(th, 2, clip_infos), rtol=0, atol=ATOL_LOG_STD)


# ---- C: promp_end_collection with a hand-written path table ------------------------------------------------------------------------

# (environment, first step, length) per task, M = 2, B = 3, S = 18 vectorised steps.  Width O + 2A = 32: a path of 1 row is 32
# elements (< 256, part of one trip of k_gather_paths), of 8 rows exactly 256, of 17 rows 544 (> 512: three trips).
GATHER_S = 18
GATHER_TABLE = [
    [(2, 0, 17),                 # its last step (17) is an unfinished tail: dropped
     (0, 0, 8), (0, 8, 1),       # two consecutive episodes of environment 0, the second of one row; steps 9.. dropped
     (1, 3, 8)],                 # environments 2, 0, 0, 1: not ordered by environment; environment 1 also drops its head
    [(4, 0, 17),
     (3, 0, 8), (3, 8, 8)],      # environment 5: no finished path at all
]


def check_gather(lib, step=0, seed=SEED64, clip_infos=False, O=20, A=6, hidden=(64, 64), hidden_act='tanh'):
    M, B, S = 2, 3, GATHER_S
    rng = np.random.RandomState(3000)
    spec = op.PolicySpec(O, A, hidden, min_std=MIN_STD, hidden_act=hidden_act)
    th = make_thetas(rng, M, O, A, hidden)
    obs = rng.randn(S, M, B, O).astype(np.float32)
    paths = [p for task in GATHER_TABLE for p in task]
    tpo = np.concatenate([[0], np.cumsum([len(task) for task in GATHER_TABLE])])
    env, start, ln = (np.array([p[j] for p in paths]) for j in range(3))
    assert all(i * B <= e < (i + 1) * B for i, task in enumerate(GATHER_TABLE) for e, _, _ in task)
    assert sorted(set(ln * (O + 2 * A))) == [32, 256, 544] and 5 not in env
    rew = rng.randn(int(ln.sum())).astype(np.float32)
    ctx = _lib.Context(M, O, A, hidden, 1, max_rows=M * B * S, max_paths=M * B * 2, lib=lib, hidden_act=hidden_act)
    try:
        ctx.set_min_std(MIN_STD)
        ctx.set_theta(th.mean(axis=0))
        ctx.set_task_thetas(th)
        ctx.begin_collection(step, B, S)
        acts = np.stack([ctx.policy_step(step, s, obs[s], seed=seed, clip_infos=clip_infos) for s in range(S)])
        # malformed tables are the library's error, and leave the collection as it was
        for bad_env, bad_start, bad_len, what in ((0, 10, 9, 'past max_steps'), (M * B, 0, 4, 'env >= M * B'), (1, 2, 0, 'len = 0')):
            e2, s2, l2 = env.copy(), start.copy(), ln.copy()
            e2[1], s2[1], l2[1] = bad_env, bad_start, bad_len
            try:
                ctx.end_collection(step, tpo, e2, s2, l2, np.zeros(int(l2.sum()), np.float32))
            except _lib.PrompError as e:
                assert 'outside the collection' in str(e), (what, str(e))
            else:
                raise AssertionError('a path %s was accepted' % what)
        ctx.end_collection(step, tpo, env, start, ln, rew)
        slab = ctx.download_step(step)
    finally:
        ctx.close()
    obs, acts = obs.reshape(S, M * B, O), acts.reshape(S, M * B, A)
    src_s = np.concatenate([s0 + np.arange(n) for s0, n in zip(start, ln)])
    src_e = np.concatenate([np.full(n, e) for e, n in zip(env, ln)])
    assert slab['obs'].shape == (int(ln.sum()), O)
    np.testing.assert_array_equal(slab['obs'], obs[src_s, src_e])
    np.testing.assert_array_equal(slab['act'], acts[src_s, src_e])
    np.testing.assert_array_equal(slab['rew'], rew)
    # means and actions against the oracle, row by row under the row's own task (the tasks hold different numbers of rows)
    task = src_e // B
    counters = src_s * (M * B) + src_e
    noise = philox.action_noise(seed, counters, A, step)
    assert_tasks_differ(spec, th, slab['obs'])
    mean_ref, m32 = np.zeros((len(task), A)), np.zeros((len(task), A), np.float32)
    for i in range(M):
        mean_ref[task == i] = op.forward(spec, th[i].astype(np.float64), slab['obs'][task == i].astype(np.float64), False)[0]
        m32[task == i] = forward32(spec, th[i], slab['obs'][task == i])
    act_ref = mean_ref + np.exp(th[task, -A:].astype(np.float64)) * noise
    a32 = helpers.fma32(np.exp(th[task, -A:]).astype(np.float32), noise, m32)
    assert maxdev(slab['old_mean'], mean_ref) <= bound(ATOL, maxdev(m32, mean_ref))
    assert maxdev(slab['act'], act_ref) <= bound(ATOL_DEVICE_NOISE, maxdev(a32, act_ref))
    np.testing.assert_allclose(slab['old_log_std'], reported_log_std(th, A, clip_infos), rtol=0, atol=ATOL_LOG_STD)


# ---- D: promp_policy_forward -------------------------------------------------------------------------------------------------------

def check_policy_forward(lib, M, batch, O, A, hidden, hidden_act='tanh', output_act=None):
    rng = np.random.RandomState(4000)
    spec = op.PolicySpec(O, A, hidden, min_std=MIN_STD, hidden_act=hidden_act, output_act=output_act or 'identity')
    th = make_thetas(rng, M, O, A, hidden)
    obs = rng.randn(M, batch, O).astype(np.float32)
    assert_tasks_differ(spec, th, obs)
    ctx = _lib.Context(M, O, A, hidden, 1, max_rows=64, max_paths=4, lib=lib, hidden_act=hidden_act, output_act=output_act)
    try:
        ctx.set_theta(th.mean(axis=0))
        ctx.set_task_thetas(th)
        got = ctx.policy_forward(obs)
    finally:
        ctx.close()
    ref = task_means(spec, th, obs)
    dev = maxdev(task_means(spec, th, obs, f32=True), ref)
    tol, err = bound(ATOL, dev), maxdev(got, ref)
    print('policy_forward %s %s: replay deviation %.2e -> bound %.2e; device %.2e' % ((M, batch, O, A), hidden, dev, tol, err))
    assert got.shape == (M, batch, A) and err <= tol, (err, tol)
