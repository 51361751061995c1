"""Start states drawn on the device (promp_draw_point_starts, promp_rollout_point_family_dev, promp_collect_point_family_dev), shared by
test_point_start_host.py (CPU), test_emu_point_start.py (emulator, the smallest case of each group) and test_gpu_point_start.py
(MI355X).  Through the C ABI, in the style of tests/point_collect_checks.py and tests/point_norm_checks.py, whose inputs, oracle loop
(collect_oracle) and events (events_of) are used as they are.

`start_table` restates the draw of promp_kernels_rollout.h (point_start_state) in NumPy on oracle.philox.philox4x32_10:
  coordinates 2 p, 2 p + 1 of the reset() under row r: counter (lo32(r), hi32(r), 0x80000000 | p, stream), key (lo32(seed), hi32(seed));
  u = ((a >> 5) 2^26 + (b >> 6)) / 2^53 from words (x, y) and (z, w); value = lo + (hi - lo) u in float64, one rounding per operation.
Every device check is BITWISE:
  a. promp_draw_point_starts against start_table.
  b. promp_collect_point_family_dev against promp_collect_point_family / _norm handed start_table's table (max_steps rows, or
     max_steps + 1 under norm): two calls on fresh contexts with the same parameters and noise; n_steps, every path table, the
     downloaded slab and, under norm, the moments.
  c. promp_rollout_point_family_dev against promp_rollout_point_family handed the [M][B][state_dim] table (row = env).
  d. the refusals, by name.
The table path is the reference here because the existing suite pins it against the NumPy environments; nothing of the kernel under
test enters an expected value.

Goal cases (b): the box +-0.015 around the origin; task 0 has zero weights and log_std -12, so its action moves the point by ~1e-7
and an episode is done at its first step exactly when its start lies in the 0.01 box, and runs to the horizon otherwise; the other
tasks get point_collect_checks.goal_case's parameters.  total_samples = M B T.  A goal case with T > 1 counts only if, on
collect_oracle fed the restated table (host test) and again on the tables the device returned (GPU test), at least one episode ends by
`done` with length < T, at least one ends by the horizon, and at least one environment starts three episodes (two of its episodes are
listed and end before the stop step, or three are listed).  With T = 1 a `done` cannot come before the horizon: that case asserts
instead that every (step, environment) up to the stop step ends an episode, and its sibling with rollouts = 3 B that every
environment starts three.  The fixed-horizon kinds (corner, walls, momentum) never report done: their cases assert that every episode
ends by the horizon, and the cases with more than one episode per environment that the second one is listed.  data_seed is chosen on
the CPU so that the events occur; no case is dropped for missing one."""
import numpy as np

from oracle import philox
from promp_amd import _lib
from tests import point_collect_checks as pc, point_family_checks as fc, point_norm_checks as pn, rollout_checks as rc
from tests.rollout_checks import MIN_STD, SEED31, SEED64

START_BIT = 0x80000000
GOAL_BOX = dict(lo=[-0.015, -0.015], hi=[0.015, 0.015])
MOMENTUM_BOX = dict(lo=[-0.2, -0.2, -0.1, -0.1], hi=[0.2, 0.2, 0.1, 0.1])
CORNER_BOX = dict(lo=[-0.2, -0.2], hi=[0.2, 0.2])
ORIGIN_BOX = dict(lo=[-2.0, -2.0], hi=[2.0, 2.0])
KIND_BOX = dict(goal=GOAL_BOX, momentum=MOMENTUM_BOX, corner=CORNER_BOX, walls=CORNER_BOX)
SLAB_KEYS = ('obs', 'act', 'rew', 'old_mean', 'old_log_std')
TABLE_KEYS = ('n_steps', 'task_path_offsets', 'path_row_offsets', 'path_env', 'path_start', 'path_len')


# ---- the draw, restated -----------------------------------------------------------------------------------------------------------

def start_counters(rows, pair, stream):
    """[len(rows), 4] uint32: the Philox counters of coordinate pair `pair` of the resets under `rows`"""
    rows = np.asarray(rows, dtype=np.uint64)
    return np.stack([(rows & np.uint64(0xFFFFFFFF)).astype(np.uint32), (rows >> np.uint64(32)).astype(np.uint32),
                     np.full(rows.size, START_BIT | pair, np.uint32), np.full(rows.size, stream, np.uint32)], axis=-1)


def start_uniform(a, b):
    """two uint32 words -> float64 in [0, 1): 27 + 26 bits, every step exact"""
    hi, lo = (a >> np.uint32(5)).astype(np.float64), (b >> np.uint32(6)).astype(np.float64)
    return (hi * 67108864.0 + lo) / 9007199254740992.0


def start_rows(seed, stream, rows, state_dim, lo, hi):
    """[len(rows), state_dim] float64: the reset() filed under every start-table row of `rows`"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    assert state_dim in (2, 4) and lo.shape == hi.shape == (state_dim,)
    rows = np.asarray(rows, dtype=np.uint64).ravel()
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    out = np.zeros((rows.size, state_dim))
    for p in range(state_dim // 2):
        w = philox.philox4x32_10(start_counters(rows, p, stream), key)
        for j, (a, b) in enumerate(((w[:, 0], w[:, 1]), (w[:, 2], w[:, 3]))):
            k = 2 * p + j
            out[:, k] = lo[k] + (hi[k] - lo[k]) * start_uniform(a, b)
    return out


def start_table(seed, stream, n_rows, n_envs, state_dim, lo, hi):
    """[n_rows, n_envs, state_dim]: row s, environment e is the reset() under r = s * n_envs + e"""
    return start_rows(seed, stream, np.arange(n_rows * n_envs), state_dim, lo, hi).reshape(n_rows, n_envs, state_dim)


def check_restatement_on_cpu():
    """host only: range, moments, the two counter domains"""
    lo, hi = np.array(MOMENTUM_BOX['lo']), np.array(MOMENTUM_BOX['hi'])
    n = 24576
    for seed, stream in ((12345, 1), (SEED64, 0)):
        t = start_rows(seed, stream, np.arange(n), 4, lo, hi)
        assert (t >= lo).all() and (t <= hi).all()
        width = hi - lo
        z_mean = (t.mean(axis=0) - (lo + hi) / 2) / (width / np.sqrt(12.0 * n))
        # variance of U(lo, hi): w^2 / 12; the sample variance's own deviation: sqrt((m4 - m2^2) / n), m4 = w^4 / 80
        z_var = (t.var(axis=0) - width ** 2 / 12) / np.sqrt((width ** 4 / 80 - width ** 4 / 144) / n)
        print('seed %#x stream %d: z of the four means %s, of the four variances %s' % (seed, stream, np.round(z_mean, 2), np.round(z_var, 2)))
        assert np.abs(z_mean).max() <= 4.0 and np.abs(z_var).max() <= 4.0, (z_mean, z_var)      # (the bound asked for is 5 sigma)
    assert np.abs((start_rows(12345, 1, np.arange(n), 4, lo, hi).mean(axis=0) - (lo + hi) / 2) / ((hi - lo) / np.sqrt(12.0 * n))).max() <= 2.4
    # u itself: below 1, and the largest words give the largest value below 1
    top = start_uniform(np.array([0xFFFFFFFF], np.uint32), np.array([0xFFFFFFFF], np.uint32))[0]
    assert top == 1.0 - 2.0 ** -53 and start_uniform(np.array([0], np.uint32), np.array([0], np.uint32))[0] == 0.0
    # lo == hi: exactly lo
    assert (start_rows(7, 0, np.arange(50), 2, [0.0, 0.25], [0.0, 0.25]) == np.array([0.0, 0.25])).all()
    # no counter of the start domain is an action-noise counter: word 2 of the noise is an action pair below 32
    rows = np.concatenate([np.arange(1000), (1 << 32) + np.arange(10)])
    for pair in (0, 1):
        assert (start_counters(rows, pair, 1)[:, 2] >= START_BIT).all()
    assert all(p < 32 for p in range((8 + 1) // 2))          # act_dim <= 8
    noise = philox.action_noise(12345, np.arange(64), 2, 1)
    assert not np.isin(start_rows(12345, 1, np.arange(64), 2, [-1, -1], [1, 1]).astype(np.float32), noise).any()
    # the stream and the high word of the seed matter
    a = start_rows(SEED64, 0, np.arange(8), 2, [-2, -2], [2, 2])
    assert np.all(a != start_rows(SEED64, 1, np.arange(8), 2, [-2, -2], [2, 2]))
    assert np.all(a != start_rows(SEED64 & 0xFFFFFFFF, 0, np.arange(8), 2, [-2, -2], [2, 2]))


# ---- a. the draw on the device ----------------------------------------------------------------------------------------------------

DRAW_CASES = [        # n_rows, n_envs, state_dim, box, seed
    (3, 7, 4, MOMENTUM_BOX, SEED31),
    (5, 130, 2, ORIGIN_BOX, SEED64),
    (2, 3, 2, dict(lo=[0.0, 0.25], hi=[0.0, 0.25]), 12345),
]


def check_draw(lib, n_rows, n_envs, state_dim, box, seed):
    ctx = _lib.Context(2, state_dim, 2, (32, 32), 1, max_rows=8, max_paths=4, lib=lib)
    try:
        got = [ctx.draw_point_starts(step, n_rows, n_envs, state_dim, box['lo'], box['hi'], seed) for step in (0, 1)]
    finally:
        ctx.close()
    for step in (0, 1):
        want = start_table(seed, step, n_rows, n_envs, state_dim, box['lo'], box['hi'])
        assert got[step].dtype == np.float64 and got[step].shape == want.shape
        assert np.array_equal(got[step], want), (step, np.abs(got[step] - want).max())
    if box['lo'] == box['hi']:
        assert (got[0] == np.array(box['lo'])).all()
    else:
        assert np.all(got[0] != got[1])                    # the step slot is the stream


# ---- b. collections ---------------------------------------------------------------------------------------------------------------

# kind, M, B, T, hidden, normalization_scale, noise, step, seed, norm flags or None, more (data_seed, rollouts, max_steps)
COLLECT_CASES = [
    ('goal', 2, 4, 1, (32, 32), 10, 'host', 0, SEED31, None, dict()),                              # every step ends an episode
    ('goal', 2, 4, 1, (32, 32), 10, 'device', 1, SEED31, (1, 1), dict(rollouts=12)),               # ... three per environment
    ('goal', 2, 3, 6, (32, 16, 24), 10, 'host', 0, SEED64, None, dict(data_seed=1)),               # layer by layer
    ('walls', 2, 3, 5, (32, 32), 10, 'host', 1, SEED31, None, dict()),
    ('walls', 2, 3, 5, (32, 32), 10, 'device', 0, SEED64, None, dict(rollouts=6)),                 # a second episode, from a drawn row
    ('corner', 2, 3, 6, (32, 16, 24), 10, 'host', 0, SEED31, (1, 0), dict()),                      # k_gen_point_norm_collect
    ('momentum', 2, 5, 5, (64, 64), 10, 'device', 1, SEED64, (1, 1), dict()),                      # two blocks per reset, the last row
    ('goal', 3, 65, 6, (32, 32), 10, 'host', 0, SEED64, None, dict()),                             # a second lane trip
    ('goal', 2, 129, 4, (64, 64), 0, 'device', 1, SEED64, None, dict()),                           # bare environment, a third trip
]
EMU_COLLECT_CASES = COLLECT_CASES[:1] + COLLECT_CASES[2:3] + COLLECT_CASES[5:6]
GOAL_EVENTS = ('done', 'horizon', 'three_episodes')


def collect_case(kind, M, B, T, hidden, normalization_scale, noise, step, seed, flags, data_seed=0, rollouts=None):
    """inputs of one case; c['start'] is the restated table for (seed, step): max_steps rows, one more under norm"""
    norm = None if flags is None else dict(normalize_obs=bool(flags[0]), normalize_reward=bool(flags[1]), obs_alpha=0.05, reward_alpha=0.2)
    N, O = M * B, pn.STATE_DIM[kind]
    if kind == 'goal':
        c = pc.goal_case(M, B, T, hidden, normalization_scale, noise, step, seed, data_seed, rollouts)
        c['th'][0] = 0.0
        c['th'][0, -2:] = -12.0
        c.update(kind=kind, N=N, O=O)
    else:
        c = pn.norm_case(kind, M, B, T, hidden, normalization_scale, noise, step, seed, data_seed, rollouts)
        c['z'] = c['z'][:c['S']]
    box = KIND_BOX[kind]
    n_rows = c['S'] + (norm is not None)
    c['start'] = start_table(seed, step, n_rows, N, O, box['lo'], box['hi'])
    c.update(box=box, norm=norm, seed=seed, step=step)
    return c


def case_events(c, tables, end_len=None):
    """the events of the module docstring on a set of tables (the oracle's or the device's)"""
    M, B, T = c['M'], c['B'], c['T']
    ln, env, start = np.asarray(tables['len']), np.asarray(tables['env']), np.asarray(tables['start'])
    stop = int(tables['stop'])
    found = set()
    if ((ln < T)).any():
        found.add('done')
    if (ln == T).any():
        found.add('horizon')
    listed = np.bincount(env, minlength=M * B)
    ends_before_stop = np.bincount(env[start + ln - 1 < stop], minlength=M * B)
    if (listed >= 3).any() or (ends_before_stop >= 2).any():
        found.add('three_episodes')
    return found


def assert_case_events(c, tables):
    found = case_events(c, tables)
    ln = np.asarray(tables['len'])
    if c['kind'] == 'goal' and c['T'] > 1:
        assert set(GOAL_EVENTS) <= found, (sorted(found), 'change data_seed')
    elif c['kind'] == 'goal':
        n_listed = (int(tables['stop']) + 1) * c['N']
        assert len(ln) == n_listed and (ln == 1).all()            # every (step, environment) up to the stop step ends an episode
        if c['total'] >= 3 * c['N']:
            assert 'three_episodes' in found
    else:
        assert (ln == c['T']).all()                               # the fixed-horizon kinds end by the horizon alone
        if c['total'] >= 2 * c['N'] * c['T']:
            assert 'three_episodes' in found or np.bincount(np.asarray(tables['env'])).max() >= 2


def oracle_tables(c):
    """CPU only: the plain oracle loop on the restated table (goal kind) -> its tables"""
    o = pc.case_oracle(c)
    assert o['tables'] is not None, 'the oracle does not reach total_samples'
    return o['tables']


def collect_case_is_sound(case):
    """CPU only.  Goal: the events on collect_oracle fed the restated table.  The other kinds end every episode at multiples of T:
    their tables follow from the shapes alone."""
    c = collect_case(*case[:-1], **case[-1])
    if c['kind'] == 'goal' and c['norm'] is None:
        assert_case_events(c, oracle_tables(c))
    elif c['kind'] == 'goal':
        # (under norm the policy sees normalised observations; with T = 1 the tables do not depend on the policy at all)
        assert c['T'] == 1
    else:
        per_env = c['total'] // (c['N'] * c['T'])
        assert c['total'] == per_env * c['N'] * c['T'] and c['S'] >= per_env * c['T']
    return c


def open_context(lib, c):
    rows = c['S'] * c['N']
    ctx = _lib.Context(c['M'], c['O'], 2, c['hidden'], 1, max_rows=rows, max_paths=rows, lib=lib)
    ctx.set_min_std(MIN_STD)
    ctx.set_theta(c['th'].mean(axis=0))
    ctx.set_task_thetas(c['th'])
    return ctx


def run_collect(lib, c, device_starts, moments=None, **over):
    """one call on a fresh context -> (tables, slab, moments after or None)"""
    kw = dict(total_samples=c['total'], max_path_length=c['T'], clip_infos=True, seed=c['seed'], norm=c['norm'], **c['env'])
    kw.update(over)
    z = c['z'] if c['noise'] == 'host' else None
    ctx = open_context(lib, c)
    try:
        if c['norm'] is not None:
            ctx.set_point_norm(moments)
        if device_starts:
            got = ctx.collect_point_family(c['step'], c['kind'], c['tasks'], None, z, starts=dict(c['box'], seed=c['seed']),
                                           envs_per_task=c['B'], max_steps=c['S'], **kw)
        else:
            got = ctx.collect_point_family(c['step'], c['kind'], c['tasks'], c['start'], z, **kw)
        slab = ctx.download_step(c['step'])
        after = ctx.get_point_norm(c['N'], c['O']) if c['norm'] is not None else None
    finally:
        ctx.close()
    return got, slab, after


def check_collect(lib, case):
    c = collect_case(*case[:-1], **case[-1])
    moments = pn.initial_moments(c['N'], c['O']) if c['norm'] is not None else None
    dev, dev_slab, dev_after = run_collect(lib, c, True, moments)
    ref, ref_slab, ref_after = run_collect(lib, c, False, moments)
    print('%s: %d steps, %d paths, lengths %s' % (case[:5], dev['n_steps'], len(dev['path_len']), np.bincount(dev['path_len']).tolist()))
    for k in TABLE_KEYS:
        assert np.array_equal(dev[k], ref[k]), (k, dev[k], ref[k])
    for k in SLAB_KEYS:
        assert dev_slab[k].shape == ref_slab[k].shape and np.array_equal(dev_slab[k], ref_slab[k]), k
    assert np.all(np.isfinite(ref_slab['act'])) and np.any(ref_slab['rew'] != 0)
    if c['norm'] is not None:
        assert np.array_equal(dev_after, ref_after) and np.any(ref_after != moments)
    # the first observation of every path is float32 of the drawn reset() (no observation normalisation), and the events occur
    if c['norm'] is None or not c['norm']['normalize_obs']:
        first = dev_slab['obs'][dev['path_row_offsets'][:-1]]
        assert np.array_equal(first, c['start'][dev['path_start'], dev['path_env']].astype(np.float32))
    assert_case_events(c, dict(len=dev['path_len'], env=dev['path_env'], start=dev['path_start'], stop=dev['n_steps'] - 1))


# ---- c. fixed-horizon rollouts ----------------------------------------------------------------------------------------------------

# kind, M, B, T, hidden, noise, step, seed
ROLLOUT_CASES = [
    ('walls', 2, 3, 4, (32, 16, 24), 'host', 0, SEED31),
    ('momentum', 2, 5, 4, (64, 64), 'device', 1, SEED64),
    ('corner', 3, 65, 5, (32, 32), 'host', 0, SEED64),
]


def check_rollout(lib, kind, M, B, T, hidden, noise, step, seed):
    if kind == 'corner':
        p = rc.point_case(M, B, T, hidden, 'dense', 10, noise, step, seed)
        c = dict(th=p['th'], tasks=p['goals'], z=p['z'], env=p['env'])
    elif kind == 'momentum':
        c = fc.momentum_case(M, B, T, hidden, 'dense_squared', 10, noise, step, seed)
    else:
        c = pn.norm_case('walls', M, B, T, hidden, 10, 'host', step, seed)
        c = dict(th=c['th'], tasks=c['tasks'], env=c['env'], z=fc.make_noise(np.random.RandomState(3), noise, M, B, T, step, seed))
    O, box = pn.STATE_DIM[kind], KIND_BOX[kind]
    start = start_table(seed, step, 1, M * B, O, box['lo'], box['hi']).reshape(M, B, O)
    z = c['z'] if noise == 'host' else None
    slabs = []
    for device_starts in (True, False):
        ctx = _lib.Context(M, O, 2, hidden, 1, max_rows=M * B * T, max_paths=M * B, lib=lib)
        try:
            ctx.set_min_std(MIN_STD)
            ctx.set_theta(c['th'].mean(axis=0))
            ctx.set_task_thetas(c['th'])
            kw = dict(noise=z, clip_infos=True, seed=seed, path_length=T, **c['env'])
            if device_starts:
                ctx.rollout_point_family(step, kind, c['tasks'], None, starts=dict(box, seed=seed), envs_per_task=B, **kw)
            else:
                ctx.rollout_point_family(step, kind, c['tasks'], start, **kw)
            slabs.append(ctx.download_step(step))
        finally:
            ctx.close()
    dev, ref = slabs
    for k in SLAB_KEYS:
        assert dev[k].shape == ref[k].shape and np.array_equal(dev[k], ref[k]), k
    assert np.array_equal(dev['obs'][::T], start.reshape(M * B, O).astype(np.float32)) and np.any(ref['rew'] != 0)


# ---- d. refusals ------------------------------------------------------------------------------------------------------------------

def check_refusals(lib):
    """by name; the step keeps no layout of the refused call, and the moments are bit for bit as they were"""
    c = collect_case('goal', 2, 3, 6, (32, 32), 10, 'host', 0, SEED31, (1, 1))
    state = pn.initial_moments(c['N'], c['O'])
    good = dict(c['box'], seed=c['seed'])

    def call_collect(ctx, starts, norm=c['norm'], **over):
        kw = dict(total_samples=c['total'], max_path_length=c['T'], clip_infos=True, seed=c['seed'], norm=norm, starts=starts,
                  envs_per_task=c['B'], max_steps=c['S'], **c['env'])
        kw.update(over)
        kind = kw.pop('kind', 'goal')
        tasks = kw.pop('tasks', c['tasks'])
        return ctx.collect_point_family(0, kind, tasks, None, c['z'][:kw['max_steps']], **kw)

    def call_rollout(ctx, starts, **over):
        kw = dict(noise=None, clip_infos=True, seed=c['seed'], path_length=4, starts=starts, envs_per_task=c['B'], normalization_scale=10.0)
        kw.update(over)
        kind = kw.pop('kind', 'corner')
        return ctx.rollout_point_family(0, kind, kw.pop('tasks', c['tasks']), None, **kw)

    def refused(ctx, call, match, *args, **kw):
        try:
            call(ctx, *args, **kw)
        except _lib.PrompError as e:
            assert match in str(e), (match, str(e))
            try:
                ctx.process_samples(0)
            except _lib.PrompError:
                pass
            else:
                raise AssertionError('the refused call left data behind')
        else:
            raise AssertionError('accepted: expected a refusal naming %r' % match)

    null = _lib.C.POINTER(_lib.PointStartOpts)()
    ctx = open_context(lib, c)
    try:
        ctx.set_point_norm(state)
        bad = [('lo = ', dict(lo=[0.1, 0.0], hi=[0.0, 0.1], seed=1)), ('lo = ', dict(lo=[0.0, 0.2], hi=[0.1, 0.1], seed=1)),
               ('not finite', dict(lo=[0.0, 0.0], hi=[np.inf, 0.1], seed=1)), ('not finite', dict(lo=[np.nan, 0.0], hi=[0.1, 0.1], seed=1)),
               ('not finite', dict(lo=[0.0, -np.inf], hi=[0.1, 0.1], seed=1))]
        for call in (call_collect, call_rollout):
            for match, starts in bad:
                refused(ctx, call, match, starts)
        # NULL starts, straight through the C ABI
        env = _lib.PointFamilyOpts(3, 0, 1, 2, 10.0, 0.1, 2.0, 0)
        opts = _lib.PointCollectOpts(env, 0.01, c['T'], c['S'], c['total'])
        tasks = np.ascontiguousarray(c['tasks'])
        n = _lib.C.c_int32(0)
        buf = [np.zeros(c['S'] * c['N'] + 1, np.int32) for _ in range(4)]
        ptr = lambda a: a.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32))
        for name, args in (('promp_collect_point_family_dev', (0, c['B'], tasks.ctypes.data_as(_lib._D), null, None, _lib.C.byref(opts), None,
                                                               _lib.C.byref(n), _lib.C.byref(n)) + tuple(ptr(b) for b in buf)),
                           ('promp_rollout_point_family_dev', (0, c['B'], 4, tasks.ctypes.data_as(_lib._D), null, None, _lib.C.byref(env))),
                           ('promp_draw_point_starts', (0, 2, 3, 2, null, tasks.ctypes.data_as(_lib._D)))):
            try:
                ctx._call(name, *args)
            except _lib.PrompError as e:
                assert 'NULL' in str(e), str(e)
            else:
                raise AssertionError('%s accepted NULL starts' % name)
        # what the table entry points refuse
        refused(ctx, call_collect, 'do not reach total_samples', good, total_samples=c['S'] * c['N'] + 1)
        refused(ctx, call_collect, 'do not reach total_samples', good, max_steps=1)
        refused(ctx, call_collect, 'max_path_length', good, max_path_length=0)
        refused(ctx, call_collect, 'unknown environment kind', good, kind=4)
        refused(ctx, call_collect, 'task_dim', good, kind=1)
        refused(ctx, call_collect, 'obs_dim', dict(MOMENTUM_BOX, seed=1), kind='momentum')
        refused(ctx, call_collect, 'obs_alpha', good, norm=dict(c['norm'], obs_alpha=1.5))
        refused(ctx, call_rollout, 'unknown environment kind', good, kind=3)
        refused(ctx, call_rollout, 'task_dim', good, kind='walls')
        refused(ctx, call_rollout, 'exceeds max_rows', good, path_length=c['S'] + 1)
        for bad_draw in (dict(n_rows=0), dict(state_dim=3), dict(lo=[0.2, 0.0]), dict(hi=[np.nan, 0.1])):
            kw = dict(step=0, n_rows=2, n_envs=3, state_dim=2, lo=[0.0, 0.0], hi=[0.1, 0.1], seed=1)
            kw.update(bad_draw)
            try:
                ctx.draw_point_starts(**kw)
            except _lib.PrompError:
                pass
            else:
                raise AssertionError('promp_draw_point_starts accepted %r' % bad_draw)
        assert np.array_equal(ctx.get_point_norm(c['N'], c['O']), state), 'a refused call moved the moments'
        # a coordinate the environment does not have is not looked at; and the same call with a sound box is accepted
        call_collect(ctx, dict(lo=[-0.015, -0.015, 1.0], hi=[0.015, 0.015, 0.0], seed=c['seed']))
        assert np.any(ctx.get_point_norm(c['N'], c['O']) != state)
        ctx.process_samples(0)
    finally:
        ctx.close()
    small = _lib.Context(c['M'], 2, 2, c['hidden'], 1, max_rows=c['S'] * c['N'], max_paths=2, lib=lib)       # refused behind the kernels
    try:
        small.set_min_std(MIN_STD)
        small.set_task_thetas(c['th'])
        small.set_point_norm(state)
        refused(small, call_collect, 'max_paths', good)
        assert np.array_equal(small.get_point_norm(c['N'], c['O']), state)
    finally:
        small.close()
