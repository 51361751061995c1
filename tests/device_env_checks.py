"""Rollouts of an environment that lives on the device (promp_policy_step_dev / promp_file_step_dev / promp_end_collection_dev /
promp_upload_step_dev, DeviceEnvSampler), shared by test_emu_device_env.py (emulator, smallest shapes) and test_gpu_device_env.py
(MI355X).  Through the C ABI, in the style of tests/point_collect_checks.py.

Every comparison is EXACT (np.testing.assert_array_equal): the device path launches the kernels of the host path on the same bits
-- the same observations, seed, Philox counter and stream word --, so nothing separates the two but where the arrays live.

The environment is `Toy`, a deterministic NumPy vectorised environment in float32: the observation is updated from the action
(so a wrong action shows in every later row), the reward depends on action, task and step, and `done` is read from a fixed table
indexed by (environment, episode, step) -- some episodes end early, some at the horizon, by a plan that `planned_end_len` restates
without running anything.  The host path steps it as DeviceSlabSampler steps its pool; the device path MIRRORS it into
DeviceArrays every step (upload the observations, download the actions, upload rewards and flags, download `ended`), which defeats
the purpose of the feature but pins its semantics.  The expected tables come from the plan alone
(point_collect_checks.tables_of: the reference's loop over an end_len table); the code under test never enters an expectation."""
import numpy as np
import pytest

from promp_amd import _lib
from tests import helpers, point_collect_checks as pc, rollout_checks as rc

SEED = rc.SEED64
EPISODES = 7


# ---- the toy environment ---------------------------------------------------------------------------------------------------------

class Toy(object):
    """n = M * B environments, environment e = task * B + b.  plan[e, k]: the step count at which episode k (mod EPISODES) of
    environment e reports done; T + 1: never (the episode ends at the horizon)."""

    def __init__(self, M, B, O, A, T, data_seed=0):
        rng = np.random.RandomState(4000 + data_seed)
        self.M, self.B, self.O, self.A, self.T, self.n = M, B, O, A, T, M * B
        self.W = rng.uniform(-1, 1, size=(A, O)).astype(np.float32)
        self.obs0 = rng.uniform(-1, 1, size=(self.n, O)).astype(np.float32)
        e, k = np.arange(self.n)[:, None], np.arange(EPISODES)[None, :]
        self.plan = 1 + (5 * e + 3 * k + (e * k) % 2) % (T + 1)
        self.task = np.zeros(M, np.float32)
        self.reset()

    def set_tasks(self, tasks):
        self.task = np.asarray(tasks, dtype=np.float32).reshape(self.M)

    def _start(self, idx):
        return (self.obs0[idx] * (np.float32(1) + np.float32(0.25) * self.episode[idx].astype(np.float32))[:, None]
                + np.float32(0.1) * self.task[idx // self.B][:, None]).astype(np.float32)

    def reset(self):
        self.episode, self.t = np.zeros(self.n, np.int64), np.zeros(self.n, np.int64)
        self.obs = self._start(np.arange(self.n))
        return self.obs.copy()

    def step(self, actions):
        a = np.asarray(actions, dtype=np.float32).reshape(self.n, self.A)
        drive = (a[:, :, None] * self.W[None, :, :]).sum(axis=1, dtype=np.float32)
        self.obs = (np.float32(0.5) * self.obs + np.float32(0.1) * np.tanh(drive)).astype(np.float32)
        rew = (np.float32(0.01) * a.sum(axis=1, dtype=np.float32) + self.t.astype(np.float32)
               - self.task[np.arange(self.n) // self.B]).astype(np.float32)
        self.t += 1
        done = self.t == self.plan[np.arange(self.n), self.episode % EPISODES]
        return self.obs.copy(), rew, done

    def reset_where(self, ended):
        idx = np.flatnonzero(np.asarray(ended))
        self.episode[idx] += 1
        self.t[idx] = 0
        self.obs[idx] = self._start(idx)
        return self.obs.copy()


def planned_end_len(toy, S):
    """end_len [S, n] from the plan alone: the length of the episode of environment e that ends at step s, else 0"""
    out = np.zeros((S, toy.n), np.int32)
    for e in range(toy.n):
        s, k = 0, 0
        while True:
            n = min(int(toy.plan[e, k % EPISODES]), toy.T)
            s += n
            if s > S:
                break
            out[s - 1, e] = n
            k += 1
    return out


def choose_total(toy, lo):
    """total_samples whose stop step s* >= lo has at least three episodes ending exactly at s*, at least one environment in the
    middle of an episode there (dropped), more rows than total_samples, an early end and a horizon end among the listed paths and
    a finished episode for every task.  From the plan alone -> (total_samples, max_steps, expected tables)"""
    S = 3 * toy.T + lo
    end_len = planned_end_len(toy, S)
    per_step = end_len.sum(axis=1)
    cum = np.cumsum(per_step)
    for s in range(lo, S - toy.T):
        total = int(cum[s - 1]) + 1                 # the smallest total that stops at s (if anything ends there)
        if (end_len[s] > 0).sum() < 3 or not (end_len[s] == 0).any():
            continue
        t = pc.tables_of(end_len, toy.M, toy.B, total)
        if t['stop'] != s or t['rows'] <= total or (np.diff(t['tpo']) == 0).any():
            continue
        if not ((t['len'] == toy.T).any() and (t['len'] < toy.T).any()):
            continue
        max_steps = pc.max_steps_of(toy.M, toy.B, toy.T, total)
        assert s < max_steps <= S
        return total, max_steps, t
    raise AssertionError('no stop step with the wanted events: change the plan')


# ---- contexts and the two loops ---------------------------------------------------------------------------------------------------

def make_ctx(lib, M, B, O, A, hidden, max_steps, data_seed=0):
    rng = np.random.RandomState(1000 + data_seed)
    th = rc.make_thetas(rng, M, O, A, hidden)
    ctx = _lib.Context(M, O, A, hidden, 1, max_rows=max_steps * M * B, max_paths=max_steps * M * B, lib=lib)
    ctx.set_min_std(rc.MIN_STD)
    ctx.set_theta(th.mean(axis=0))
    ctx.set_task_thetas(th)
    return ctx


def host_collection(ctx, toy, step, max_steps, total, seed, clip_infos):
    """DeviceSlabSampler's loop (samplers/device_slab_sampler.py) on the toy -> dict(tables, slab, actions [s], ended [s])"""
    M, B, O, A, T, n = toy.M, toy.B, toy.O, toy.A, toy.T, toy.n
    ctx.begin_collection(step, B, max_steps)
    rewards = np.zeros((max_steps, n), np.float32)
    started, length = np.zeros(n, np.int64), np.zeros(n, np.int64)
    done_paths, actions, ends = [[] for _ in range(M)], [], []
    collected, s = 0, 0
    obs = toy.reset()
    while collected < total:
        assert s < max_steps
        a = ctx.policy_step(step, s, obs.reshape(M, B, O), seed=seed, clip_infos=clip_infos).reshape(n, A)
        actions.append(a.copy())
        _, rewards[s], done = toy.step(a)
        length += 1
        ended = done | (length >= T)
        for env in np.flatnonzero(ended):
            done_paths[env // B].append((env, int(started[env]), int(length[env])))
            collected += int(length[env])
            started[env] = s + 1
        length[ended] = 0
        obs = toy.reset_where(ended)
        ends.append(ended.astype(np.uint8))
        s += 1
    flat = [p for tp in done_paths for p in tp]
    tpo = np.concatenate([[0], np.cumsum([len(tp) for tp in done_paths])]).astype(np.int32)
    env_of, start_of, len_of = (np.array([p[k] for p in flat], np.int32) for k in range(3))
    ctx.end_collection(step, tpo, env_of, start_of, len_of,
                       np.concatenate([rewards[a0:a0 + k, e] for e, a0, k in zip(env_of, start_of, len_of)]))
    tables = dict(n_steps=s, task_path_offsets=tpo, path_env=env_of, path_start=start_of, path_len=len_of,
                  path_row_offsets=np.concatenate([[0], np.cumsum(len_of)]).astype(np.int32))
    return dict(tables=tables, slab=ctx.download_step(step), actions=actions, ended=ends)


class Mirror(object):
    """the toy behind DeviceArrays: the vec_env protocol of samplers/device_env_sampler.py, one upload / download per array and step"""

    def __init__(self, ctx, toy):
        self.ctx, self.toy, self.n_envs = ctx, toy, toy.n
        self.obs = ctx.device_array((toy.n, toy.O), np.float32)
        self.rew = ctx.device_array((toy.n,), np.float32)
        self.done = ctx.device_array((toy.n,), np.uint8)
        self.seen_actions, self.seen_ended = [], []

    def set_tasks(self, tasks):
        self.toy.set_tasks(tasks)

    def reset(self):
        return self.obs.upload(self.toy.reset())

    def step(self, actions):
        a = actions.download()
        self.seen_actions.append(a.copy())
        obs, rew, done = self.toy.step(a)
        return self.obs.upload(obs), self.rew.upload(rew), self.done.upload(done.astype(np.uint8))

    def reset_where(self, ended):
        e = ended.download()
        self.seen_ended.append(e.copy())
        return self.obs.upload(self.toy.reset_where(e))


def device_collection(ctx, toy, step, max_steps, total, seed, clip_infos, n_steps, early_end_at=None):
    """the device path over the mirrored toy for n_steps vectorised steps -> as host_collection, plus progress [s]: what
    collection_progress reported after filing step s.  early_end_at: a step after whose filing end_collection_dev is tried and must
    refuse with the collection left open."""
    M, B, T, n = toy.M, toy.B, toy.T, toy.n
    env = Mirror(ctx, toy)
    actions, ended = ctx.device_array((n, toy.A), np.float32), ctx.device_array((n,), np.uint8)
    ctx.begin_collection(step, B, max_steps)
    progress = []
    obs = env.reset()
    for s in range(n_steps):
        ctx.policy_step_dev(step, s, obs, actions, seed=seed, clip_infos=clip_infos)
        _, rew, done = env.step(actions)
        ctx.file_step_dev(step, s, rew, done, T, ended)
        progress.append(ctx.collection_progress(step, total))
        if early_end_at is not None and s == early_end_at:
            with pytest.raises(_lib.PrompError, match='do not reach total_samples'):
                ctx.end_collection_dev(step, total)
        obs = env.reset_where(ended)
    tables = ctx.end_collection_dev(step, total)
    return dict(tables=tables, slab=ctx.download_step(step), actions=env.seen_actions, ended=env.seen_ended, progress=progress)


def assert_same_collection(a, b):
    for k in ('n_steps',):
        assert a['tables'][k] == b['tables'][k], (k, a['tables'][k], b['tables'][k])
    for k in ('task_path_offsets', 'path_row_offsets', 'path_env', 'path_start', 'path_len'):
        np.testing.assert_array_equal(a['tables'][k], b['tables'][k], err_msg=k)
    for k in ('obs', 'act', 'rew', 'old_mean', 'old_log_std'):
        assert a['slab'][k].shape == b['slab'][k].shape, k
        np.testing.assert_array_equal(a['slab'][k].view(np.uint32), b['slab'][k].view(np.uint32), err_msg=k)
    n = a['tables']['n_steps']
    assert len(a['actions']) >= n and len(b['actions']) >= n and len(a['ended']) >= n and len(b['ended']) >= n
    for s in range(n):
        np.testing.assert_array_equal(a['actions'][s].view(np.uint32), b['actions'][s].view(np.uint32), err_msg='actions of step %d' % s)
        np.testing.assert_array_equal(a['ended'][s], b['ended'][s], err_msg='ended at step %d' % s)


def assert_expected_tables(tables, want):
    assert tables['n_steps'] == want['stop'] + 1
    np.testing.assert_array_equal(tables['task_path_offsets'], want['tpo'])
    np.testing.assert_array_equal(tables['path_env'], want['env'])
    np.testing.assert_array_equal(tables['path_start'], want['start'])
    np.testing.assert_array_equal(tables['path_len'], want['len'])
    assert int(tables['path_row_offsets'][-1]) == want['rows']


# ---- 1: host loop against device path ---------------------------------------------------------------------------------------------

def check_host_against_device(lib, M, B, T, hidden, O=3, A=2, step=0, clip_infos=True):
    toy_h, toy_d = Toy(M, B, O, A, T), Toy(M, B, O, A, T)
    tasks = np.linspace(-1.0, 1.0, M)
    toy_h.set_tasks(tasks)
    toy_d.set_tasks(tasks)
    total, max_steps, want = choose_total(toy_h, lo=T)
    ctx_h, ctx_d = make_ctx(lib, M, B, O, A, hidden, max_steps), make_ctx(lib, M, B, O, A, hidden, max_steps)
    try:
        host = host_collection(ctx_h, toy_h, step, max_steps, total, SEED, clip_infos)
        assert_expected_tables(host['tables'], want)
        dev = device_collection(ctx_d, toy_d, step, max_steps, total, SEED, clip_infos, host['tables']['n_steps'])
        assert_expected_tables(dev['tables'], want)
        assert_same_collection(host, dev)
        # the horizon is the library's rule on the device path: it flagged what the host loop ended on its own
        assert any(e.any() and not e.all() for e in dev['ended'])
    finally:
        ctx_h.close()
        ctx_d.close()


# ---- 2: fixed-horizon mode -------------------------------------------------------------------------------------------------------

def check_fixed_horizon(lib, M=2, B=3, T=5, O=3, A=2, hidden=(32, 32), step=1, clip_infos=False):
    toy_h, toy_d = Toy(M, B, O, A, T + 1), Toy(M, B, O, A, T + 1)
    n = M * B
    ctx_h, ctx_d = make_ctx(lib, M, B, O, A, hidden, T), make_ctx(lib, M, B, O, A, hidden, T)
    try:
        ctx_h.begin_rollout(step, B, T)
        obs, rew = toy_h.reset(), np.zeros((n, T), np.float32)
        acts_h = []
        for t in range(T):
            a = ctx_h.policy_step(step, t, obs.reshape(M, B, O), seed=SEED, clip_infos=clip_infos).reshape(n, A)
            acts_h.append(a.copy())
            obs, rew[:, t], _ = toy_h.step(a)
        ctx_h.set_rewards(step, rew.reshape(-1))
        slab_h = ctx_h.download_step(step)

        env = Mirror(ctx_d, toy_d)
        actions, ended = ctx_d.device_array((n, A), np.float32), ctx_d.device_array((n,), np.uint8)
        ctx_d.begin_rollout(step, B, T)
        obs = env.reset()
        for t in range(T):
            ctx_d.policy_step_dev(step, t, obs, actions, seed=SEED, clip_infos=clip_infos)
            obs, r, done = env.step(actions)
            ctx_d.file_step_dev(step, t, r, done, 0, ended)          # (done is not read here; the toy's table says True somewhere)
            np.testing.assert_array_equal(ended.download(), np.full(n, 1 if t == T - 1 else 0, np.uint8))
        slab_d = ctx_d.download_step(step)
        for k in slab_h:
            np.testing.assert_array_equal(slab_h[k].view(np.uint32), slab_d[k].view(np.uint32), err_msg=k)
        for t in range(T):
            np.testing.assert_array_equal(acts_h[t].view(np.uint32), env.seen_actions[t].view(np.uint32))
        with pytest.raises(_lib.PrompError, match='outside'):           # the horizon is the slab's: there is no step T
            ctx_d.file_step_dev(step, T, r, done, 0, ended)
    finally:
        ctx_h.close()
        ctx_d.close()


# ---- 3: promp_upload_step_dev against promp_upload_step ---------------------------------------------------------------------------

def check_upload_step_dev(lib, O=4, A=3, hidden=(32, 32), lengths=((3, 1, 5), (2, 6))):
    M = len(lengths)
    rng = np.random.RandomState(77)
    th = rc.make_thetas(rng, M, O, A, hidden)
    paths = helpers.make_paths_with_lengths(rng, th[0], lengths, O, A, hidden)
    fl = _lib.flatten_paths(paths)
    rows, n_paths = int(fl['path_row_offsets'][-1]), len(fl['path_row_offsets']) - 1
    rew = np.ascontiguousarray(fl['rew'], dtype=np.float32)
    out = []
    for dev in (False, True):
        ctx = _lib.Context(M, O, A, hidden, 1, max_rows=rows, max_paths=n_paths, lib=lib)
        try:
            ctx.set_theta(th[0])
            if dev:
                up = lambda a: ctx.device_array(a.shape, np.float32).upload(a)
                arrays = [up(np.asarray(fl[k], np.float32)) for k in ('obs', 'act', 'old_mean', 'old_log_std')] + [up(rew)]
                ctx.upload_step_dev(0, fl['task_path_offsets'], fl['path_row_offsets'], arrays[0], arrays[4], arrays[1], arrays[2],
                                    arrays[3], log_std_per_row=True)
            else:
                ctx.upload_step(0, fl['task_path_offsets'], fl['path_row_offsets'], fl['obs'], rew, fl['act'], fl['old_mean'],
                                fl['old_log_std'])
            slab = ctx.download_step(0)
            ctx.process_samples(0, discount=0.97, gae_lambda=0.9, normalize_adv=True)
            proc = {k: np.array(v) for k, v in ctx.download_processed(0).items()}
            out.append((slab, proc))
        finally:
            ctx.close()
    (slab_h, proc_h), (slab_d, proc_d) = out
    np.testing.assert_array_equal(slab_h['obs'], np.asarray(fl['obs'], np.float32))
    for k in slab_h:
        np.testing.assert_array_equal(slab_h[k].view(np.uint32), slab_d[k].view(np.uint32), err_msg=k)
    assert set(proc_h) == set(proc_d)
    for k in proc_h:
        np.testing.assert_array_equal(proc_h[k], proc_d[k], err_msg=k)
    assert np.isfinite(proc_h['advantages']).all() and np.ptp(proc_h['advantages']) > 0


# ---- 4: stop and progress ---------------------------------------------------------------------------------------------------------

def check_stop_and_progress(lib, M=2, B=3, T=4, O=3, A=2, hidden=(32, 32), step=0):
    toys = [Toy(M, B, O, A, T) for _ in range(2)]
    total, max_steps, want = choose_total(toys[0], lo=T)
    stop = want['stop']
    n_steps = min(stop + 3, max_steps)             # steps filed beyond the stop step are ignored
    assert n_steps > stop + 1 and stop >= 2
    ctxs = [make_ctx(lib, M, B, O, A, hidden, max_steps) for _ in range(2)]
    try:
        plain = device_collection(ctxs[0], toys[0], step, max_steps, total, SEED, True, n_steps)
        early = device_collection(ctxs[1], toys[1], step, max_steps, total, SEED, True, n_steps, early_end_at=stop - 1)
        for run in (plain, early):
            assert run['progress'][:stop] == [(-1, 0)] * stop
            assert run['progress'][stop:] == [(stop, want['rows'])] * (n_steps - stop)
            assert_expected_tables(run['tables'], want)
        assert_same_collection(plain, early)
        # an ended collection is closed: nothing more is filed, asked or ended
        for call in (lambda: ctxs[0].collection_progress(step, total), lambda: ctxs[0].end_collection_dev(step, total)):
            with pytest.raises(_lib.PrompError, match='promp_begin_collection has not been called'):
                call()
    finally:
        for c in ctxs:
            c.close()


# ---- 5: refusals ------------------------------------------------------------------------------------------------------------------

def check_refusals(lib, emulated, M=2, B=3, T=4, O=3, A=2, hidden=(32, 32), step=0):
    """emulated: the library is the kernel emulator, whose device is the host's heap: its pointer check passes every non-NULL pointer
    (promp_device.h), so a pageable address is refused on the real device only"""
    n = M * B
    ctx = make_ctx(lib, M, B, O, A, hidden, 2 * T)
    try:
        obs, act = ctx.device_array((n, O), np.float32).upload(np.zeros((n, O))), ctx.device_array((n, A), np.float32)
        rew, done, ended = ctx.device_array((n,), np.float32).upload(np.zeros(n)), ctx.device_array((n,), np.uint8).upload(np.zeros(n)), \
            ctx.device_array((n,), np.uint8)
        ctx._rollout_shape = (B, 2 * T)                  # (what begin_collection would have noted: the library itself must refuse)
        with pytest.raises(_lib.PrompError, match='has not been called'):
            ctx.policy_step_dev(step, 0, obs, act)
        with pytest.raises(_lib.PrompError, match='has not been called'):
            ctx.file_step_dev(step, 0, rew, done, T, ended)
        ctx.begin_collection(step, B, 2 * T)
        with pytest.raises(_lib.PrompError, match='before its policy step'):
            ctx.file_step_dev(step, 0, rew, done, T, ended)
        ctx.policy_step_dev(step, 0, obs, act, seed=SEED)
        ctx.policy_step_dev(step, 1, obs, act, seed=SEED)
        ctx.policy_step_dev(step, 2, obs, act, seed=SEED)
        with pytest.raises(_lib.PrompError, match='out of order'):
            ctx.file_step_dev(step, 1, rew, done, T, ended)
        ctx.file_step_dev(step, 0, rew, done, T, ended)
        with pytest.raises(_lib.PrompError, match='already been filed'):
            ctx.file_step_dev(step, 0, rew, done, T, ended)
        with pytest.raises(_lib.PrompError, match='out of order'):
            ctx.file_step_dev(step, 2, rew, done, T, ended)
        ctx.file_step_dev(step, 1, rew, None, T, None)               # done and ended_out may each be NULL
        ctx.file_step_dev(step, 2, rew, done, T, None)
        with pytest.raises(_lib.PrompError, match='before its policy step'):
            ctx.file_step_dev(step, 3, rew, done, T, ended)
        ctx.policy_step_dev(step, 3, obs, act, seed=SEED)
        with pytest.raises(_lib.PrompError, match='max_path_length'):
            ctx.file_step_dev(step, 3, rew, done, 0, ended)
        # NULL pointers, by name, before anything is enqueued
        for call, name in ((lambda: ctx.policy_step_dev(step, 3, 0, act), 'd_obs is NULL'),
                           (lambda: ctx.policy_step_dev(step, 3, obs, 0), 'd_actions is NULL'),
                           (lambda: ctx.file_step_dev(step, 3, 0, done, T, ended), 'd_rewards is NULL'),
                           (lambda: ctx.upload_step_dev(step, [0, 1, 2], [0, 3, 6], 0, rew), 'obs is NULL'),
                           (lambda: ctx.check_device_pointer(0), 'pointer is NULL')):
            with pytest.raises(_lib.PrompError, match=name):
                call()
        # the pointer check alone -- never an entry point that could launch -- on pageable host memory
        pageable = np.zeros(64, np.float32)
        if emulated:
            ctx.check_device_pointer(pageable.ctypes.data)
        else:
            with pytest.raises(_lib.PrompError, match='cannot read'):
                ctx.check_device_pointer(pageable.ctypes.data)
        pinned = _lib.pinned_empty(lib, (64,), np.float32)
        ctx.check_device_pointer(pinned.ctypes.data)
        ctx.check_device_pointer(obs.ptr)
        # the extractor refuses what is not device memory, by name, without calling the library
        with pytest.raises(_lib.PrompError, match='ndarray is not device memory'):
            ctx.policy_step_dev(step, 3, pageable, act)
        with pytest.raises(_lib.PrompError, match='dtype'):
            ctx.file_step_dev(step, 3, rew, rew, T, ended)
        with pytest.raises(_lib.PrompError, match='elements'):
            ctx.file_step_dev(step, 3, obs, done, T, ended)
    finally:
        ctx.close()


# ---- 6: the sampler ----------------------------------------------------------------------------------------------------------------

class ToyTasks(object):
    """what DeviceSlabSampler / DeviceEnvSampler ask of `env`: the tasks (the pool is replaced by the toy's)"""
    def sample_tasks(self, n): return list(np.random.uniform(-1, 1, size=n))
    def set_task(self, task): pass
    def reset(self): return np.zeros(1)
    def step(self, a): return np.zeros(1), 0.0, False, {}


class HostPool(object):
    """the toy as MetaSampler's pool: the horizon folded into `done`, an ended environment reset on the spot"""
    def __init__(self, toy):
        self.toy, self.length = toy, np.zeros(toy.n, np.int64)
    num_envs = property(lambda self: self.toy.n)
    def set_tasks(self, tasks): self.toy.set_tasks(tasks)
    def reset(self):
        self.length[:] = 0
        return list(self.toy.reset())
    def step(self, actions):
        _, rew, done = self.toy.step(np.asarray(actions, np.float32))
        self.length += 1
        ended = done | (self.length >= self.toy.T)
        self.length[ended] = 0
        return list(self.toy.reset_where(ended)), list(rew), ended.tolist(), [{} for _ in range(self.toy.n)]


def check_sampler(lib, M=2, B=3, T=4, O=3, A=2, hidden=(32, 32), rollouts=None, poll_every=2):
    from promp_amd.baselines.linear_baseline import LinearFeatureBaseline
    from promp_amd.policies.meta_gaussian_mlp_policy import MetaGaussianMLPPolicy
    from promp_amd.samplers.device_env_sampler import DeviceEnvSampler
    from promp_amd.samplers.device_slab_sampler import DeviceSlabSampler
    from promp_amd.samplers.meta_sample_processor import MetaSampleProcessor
    rollouts = rollouts or B
    np.random.seed(11)
    policy = MetaGaussianMLPPolicy(name='p', obs_dim=O, action_dim=A, meta_batch_size=M, hidden_sizes=hidden)
    policy.switch_to_pre_update()
    slab_sampler = DeviceSlabSampler(env=ToyTasks(), policy=policy, rollouts_per_meta_task=rollouts, meta_batch_size=M,
                                     max_path_length=T, envs_per_task=B)
    toy_h, toy_d = Toy(M, B, O, A, T), Toy(M, B, O, A, T)
    slab_sampler.vec_env = HostPool(toy_h)
    state = np.random.get_state()
    slab_sampler.update_tasks()
    want = slab_sampler.obtain_samples()
    n_envs, total = M * B, M * rollouts * T
    max_steps = T - 1 + -(-total // n_envs)
    proc = MetaSampleProcessor(baseline=LinearFeatureBaseline(), discount=0.99, gae_lambda=1, normalize_adv=True)
    before = list(policy.session.upload_serial)
    fields = ('advantages', 'returns', 'observations', 'actions', 'rewards')
    sd_want = [{k: np.array(sd[k]) for k in fields} for sd in proc.process_samples(want)]
    assert policy.session.upload_serial == before        # found resident: nothing was uploaded
    # the step slot is the Philox stream word: the second collection goes to the slot of the first (K + 1 = 2 slots, one skipped)
    policy.session.next_slot()
    ctx = policy.session.ensure(max_steps * n_envs, max_steps * n_envs)
    env_sampler = DeviceEnvSampler(Mirror(ctx, toy_d), ToyTasks(), policy, rollouts, M, T, envs_per_task=B, poll_every=poll_every)
    np.random.set_state(state)                       # the same NumPy draws: tasks, then the seed of the sampling step
    env_sampler.update_tasks()
    got = env_sampler.obtain_samples()
    assert policy.session.ctx is ctx
    assert env_sampler.last_seed is not None and env_sampler.total_timesteps_sampled == total == slab_sampler.total_timesteps_sampled
    assert env_sampler.last_n_steps <= env_sampler.last_steps_filed <= max_steps
    assert list(got.keys()) == list(want.keys()) == list(range(M))
    some_short = False
    for i in range(M):
        assert len(got[i]) == len(want[i]) > 0
        for p, q in zip(got[i], want[i]):
            for k in ('observations', 'actions', 'rewards'):
                assert p[k].shape == q[k].shape
                np.testing.assert_array_equal(p[k].view(np.uint32), q[k].view(np.uint32), err_msg=k)
            for k in ('mean', 'log_std'):
                np.testing.assert_array_equal(p['agent_infos'][k], q['agent_infos'][k], err_msg=k)
            assert p['env_infos'] == {}
            some_short |= len(p['rewards']) < T
    assert some_short
    for k in ('task_path_offsets', 'path_row_offsets', 'path_env', 'path_start'):
        np.testing.assert_array_equal(got.flat[k], want.flat[k], err_msg=k)
    before = list(policy.session.upload_serial)
    sd_got = proc.process_samples(got)
    assert policy.session.upload_serial == before
    for a, b in zip(sd_got, sd_want):
        for k in fields:
            np.testing.assert_array_equal(np.asarray(a[k]), b[k], err_msg=k)


# ---- 7: a torch environment on a stream of its own (GPU only) ----------------------------------------------------------------------

def check_torch(M=3, B=5, T=8, hidden=(32, 32)):
    """promp_amd/envs/torch_point_env.py through DeviceEnvSampler on a non-default torch stream, against the same environment stepped
    with observations and actions copied through the host for promp_policy_step: equal tables and slabs.  The caller has checked
    that torch is importable and sees the GPU."""
    import importlib.util
    import os
    import torch
    from oracle import policy as op
    from promp_amd.envs.point_env import MetaPointEnvV2
    from promp_amd.envs.torch_point_env import TorchPointVecEnv
    from promp_amd.policies.meta_gaussian_mlp_policy import MetaGaussianMLPPolicy
    from promp_amd.samplers.device_env_sampler import DeviceEnvSampler
    from promp_amd.utils import logger
    np.random.seed(3)
    n, O, A = M * B, 2, 2
    policy = MetaGaussianMLPPolicy(name='p', obs_dim=O, action_dim=A, meta_batch_size=M, hidden_sizes=hidden)
    spec = op.PolicySpec(O, A, hidden)
    theta = spec.from_ordered_dict(policy.get_param_values())
    theta[-2:] = np.log(0.02)              # steps of the box's size: some episodes end back at the origin, most at the horizon
    policy.set_params(spec.to_ordered_dict(theta))
    policy.switch_to_pre_update()
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0 and stream != torch.cuda.current_stream()
    vec_env = TorchPointVecEnv(M, B, stream=stream)
    task_env = MetaPointEnvV2()                                    # (its constructor draws a goal: built before the state is noted)
    sampler = DeviceEnvSampler(vec_env, task_env, policy, B, M, T, poll_every=2)
    state = np.random.get_state()
    sampler.update_tasks()
    got = sampler.obtain_samples()
    np.random.set_state(state)
    tasks = task_env.sample_tasks(M)                               # the same draws
    ctx, slot, total = policy.session.ctx, got.device_ref[2], M * B * T
    max_steps = T - 1 + -(-total // n)
    slab_dev = ctx.download_step(slot)
    lens = np.diff(got.flat['path_row_offsets'])
    assert (lens == T).any() and (lens < T).any() and int(lens.sum()) >= total

    # the same environment, every step through the host (DeviceSlabSampler's loop)
    env = TorchPointVecEnv(M, B, stream=torch.cuda.Stream())
    env.set_tasks(tasks)
    ctx.begin_collection(slot, B, max_steps)
    rewards = np.zeros((max_steps, n), np.float32)
    started, length = np.zeros(n, np.int64), np.zeros(n, np.int64)
    done_paths, collected, s = [[] for _ in range(M)], 0, 0

    def to_host(t):
        with torch.cuda.stream(env.stream):
            h = t.cpu()
        env.stream.synchronize()
        return h.numpy()

    obs = env.reset()
    while collected < total:
        a = ctx.policy_step(slot, s, to_host(obs).reshape(M, B, O), seed=sampler.last_seed, clip_infos=True).reshape(n, A)
        with torch.cuda.stream(env.stream):
            a_dev = torch.from_numpy(a).to(env.device)
        _, rew, done = env.step(a_dev)
        rewards[s] = to_host(rew)
        length += 1
        ended = (to_host(done) != 0) | (length >= T)
        for e in np.flatnonzero(ended):
            done_paths[e // B].append((e, int(started[e]), int(length[e])))
            collected += int(length[e])
            started[e] = s + 1
        length[ended] = 0
        with torch.cuda.stream(env.stream):
            ended_dev = torch.from_numpy(ended.astype(np.uint8)).to(env.device)
        obs = env.reset_where(ended_dev)
        s += 1
    flat = [p for tp in done_paths for p in tp]
    tpo = np.concatenate([[0], np.cumsum([len(tp) for tp in done_paths])]).astype(np.int32)
    env_of, start_of, len_of = (np.array([p[k] for p in flat], np.int32) for k in range(3))
    ctx.end_collection(slot, tpo, env_of, start_of, len_of,
                       np.concatenate([rewards[a0:a0 + k, e] for e, a0, k in zip(env_of, start_of, len_of)]))
    slab_host = ctx.download_step(slot)
    assert sampler.last_n_steps == s
    np.testing.assert_array_equal(got.flat['task_path_offsets'], tpo)
    np.testing.assert_array_equal(got.flat['path_env'], env_of)
    np.testing.assert_array_equal(got.flat['path_start'], start_of)
    np.testing.assert_array_equal(np.diff(got.flat['path_row_offsets']), len_of)
    for k in slab_host:
        assert slab_host[k].shape == slab_dev[k].shape, k
        np.testing.assert_array_equal(slab_host[k].view(np.uint32), slab_dev[k].view(np.uint32), err_msg=k)

    # two iterations of the run script's loop
    path = os.path.join(helpers.ROOT, 'run_scripts', 'pro-mp_run_torch_point_mass.py')
    mod_spec = importlib.util.spec_from_file_location('run_torch_point_mass', path)
    script = importlib.util.module_from_spec(mod_spec)
    mod_spec.loader.exec_module(script)
    logger.configure(dir=None, snapshot_mode='last', quiet=True)
    rounds, orig = [], logger.dumpkvs

    def grab():
        rounds.append(dict(logger.getkvs()))
        return orig()
    logger.dumpkvs = grab
    try:
        cfg = dict(script.DEFAULT, n_itr=2, meta_batch_size=3, rollouts_per_meta_task=4, max_path_length=10, num_promp_steps=2, poll_every=3)
        trained = script.main(cfg)
    finally:
        logger.dumpkvs = orig
    assert len(rounds) == 2 and rounds[-1]['n_timesteps'] == 2 * 2 * 3 * 4 * 10
    for kvs in rounds:
        for k in ('Step_0-AverageReturn', 'Step_1-AverageReturn', 'LossBefore', 'LossAfter'):
            assert k in kvs and np.isfinite(kvs[k]), k
    assert all(np.all(np.isfinite(v)) for v in trained.get_param_values().values())
