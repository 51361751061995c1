"""The two count axes nearly every buffer and loop depends on -- inner steps K and tasks M -- past the values of the BASELINE
configs, shared by test_gpu_count_axes.py (MI355X), test_emu_count_axes.py (emulator, four cases) and test_count_axes_host.py (the
conditions on the inputs, oracle alone).

K.  check_dims accepts num_inner_steps 1 .. PROMP_ETA_MAX = 8; sized or indexed by K are AdamArgs::eta[8] (by value), filled[8] and
slab[9] of enqueue_meta_on, the statistics row [K + 2] and its page-locked copy, scal_inner [K][M][2], the adaptation chain
(K + 1) M Theta, ginner K M Theta with k_step_size_grad's `first` flag at k == K - 1, the exchange columns red[Theta + 1 + k] and the
primal cache of every slab.  The other test files stop at K = 3 (the step-size checks at 2).  Here: K = 4 and K = 8 on one shape per
pass-kernel family (K_SHAPES), two tasks of 37 and 33 rows in two and one paths (K_LENGTHS), alpha 0.1, eta = helpers.eta_for(K).

M.  final_quarter_sum (promp_kernels_policy.h) walks 48 tasks per trip, 12 per quarter, clamped and masked: M = 48 is exactly one
trip, 49 a second trip that holds one task with the other three quarters clamped, 97 a third.  build_step_tables (promp_plan.h) floors
every task to one work item when tasks outnumber compute units, its tables then approach max_work = 2 n_cus + M, and every chain
workgroup changes task mid-launch: M = n_cus + 1 and 2 n_cus + 1, n_cus read from the device with PROMP_MAX_CUS unset (257 and 513 on
the MI355X), also take the kernels whose grid is M workgroups (or grid.y = M) past a few dozen tasks.  Inputs: K = 1, every task one
path of m_lengths(M) rows (1 .. 20, RandomState(M)), seed 900 + M.

Conditions on the inputs (test_count_axes_host.py, float64 oracle alone): the K inner KLs differ pairwise by more than 1e-3
relative and eta is pairwise different, so a permuted, truncated or repeated statistics or penalty entry moves the loss by more
than ten times its tolerance; the float64 meta-gradient of a K-axis case moves by less than 1e-5 of its max-norm under one float32
rounding of the parameters (alpha = 0.1 through eight steps diverges under some seeds, DiCE's chain through four under most: such
inputs cannot be judged at 1e-4 in float32, check_inputs_tell_the_steps_apart); leaving any one of tasks 0, 47, 48, M - 1 out of
the mean moves the meta-gradient by at least 1e-3 of its max-norm, ten times the tolerance (the loss alone is not sensitive enough
at 513 tasks: the gradient is the judge).  A seed that misses a condition is replaced by the next that meets it, never the bound.

Comparisons and tolerances are the reused checks' own (parity_checks, step_size_checks, outer_optimizer_checks, minibatch_checks,
rollout_checks, dice_shape_checks): loss and KL rtol 1e-4 / atol 1e-6, gradients, products and adapted parameters 1e-4 of the
max-norm, assert_adam_trajectory's rule, bit for bit between routes.  No new number.  Every oracle comparison passes a `worst` dict
and prints it (profiles/count_axes.txt keeps a run's figures).
"""
import functools
import os

import numpy as np

from oracle import policy as op, promp as pm
from promp_amd import _lib
from tests import dice_shape_checks as ds, fused_checks as fc, helpers, minibatch_checks as mb
from tests import parity_checks as pc, point_collect_checks as gc, step_size_checks as sc
from tests.layered_checks import report

CLIP = 0.3
ALPHA = 0.1

# ---- K axis ------------------------------------------------------------------------------------------------------------------------
K_SHAPES = {
    'chain': dict(hidden=(32, 32), O=4, A=2, family='Chain'),                  # k_pass / k_chain_hvp
    'coop_fp32': dict(hidden=(64, 64), O=33, A=3, family='CoopFp32'),          # k_wide_*
    'coop_split': dict(hidden=(128, 128), O=20, A=8, family='CoopSplit'),      # k_wb_*
    'layered': dict(hidden=(48, 40, 24), O=9, A=3, family='Layered'),          # k_gen_*
}
K_LENGTHS = [[17, 20], [33]]         # 37 rows in two paths, 33 in one: two and three 16-row tiles, partial last tiles
K_VALUES = (4, 8)
K_SEED = 940                         # + 10 * index of the shape + K


# (shape, K): the first later seed, where that one fails check_inputs_tell_the_steps_apart.  Under 958 the chain of the (64, 64) shape
# diverges through eight steps (oracle inner KLs 1612, 2207, 3266): its float64 gradient moves by 6e-5 under float32 rounding alone
_K_SEEDS = {('coop_fp32', 8): 959}


def k_seed(shape, K):
    return _K_SEEDS.get((shape, K), K_SEED + 10 * sorted(K_SHAPES).index(shape) + K)


def shape_kwargs(shape, lengths):
    """the arguments of parity_checks' comparisons for K_SHAPES[shape] on explicit path lengths; the shape's family is asserted as
    fused_checks.shape_kwargs / layered_checks.shape_kwargs assert it: a changed dispatch fails here instead of quietly running
    another family"""
    s = K_SHAPES[shape]
    if s['family'] == 'Layered':
        assert helpers.runs_layer_by_layer(s['O'], s['A'], s['hidden']), s
        return dict(M=len(lengths), P=None, T=None, O=s['O'], A=s['A'], hidden=tuple(s['hidden']), lengths_per_task=lengths)
    return fc.shape_kwargs(lengths, **s)


def run(label, fn, lib, seed, **kw):
    """fn(lib, seed, worst=..., **kw); the worst figures are printed whether it passes or not"""
    worst = {}
    try:
        fn(lib, seed, worst=worst, **kw)
    finally:
        report(label, worst, 'count_axes')
    return worst


def check_meta_k(lib, shape, K, epochs=2):
    """check_meta: the meta-gradient, all K + 2 statistics, _adapt, two Adam epochs and the trajectory"""
    return run('K=%d %s meta' % (K, shape), pc.check_meta, lib, k_seed(shape, K), K=K, epochs=epochs, **shape_kwargs(shape, K_LENGTHS))


def check_primal_cache_k(lib, K=8, shape='chain'):
    return run('K=%d %s primal_cache' % (K, shape), pc.check_primal_cache, lib, k_seed(shape, K), K=K, **shape_kwargs(shape, K_LENGTHS))


def ragged_kwargs(shape):
    """M 2, two ragged paths of at most 20 rows per task, for the checks that draw their own paths (helpers.make_promp_case)"""
    kw = shape_kwargs(shape, K_LENGTHS)
    return dict(M=2, P=2, T=20, O=kw['O'], A=kw['A'], hidden=kw['hidden'])


# DiCE: N(0, 1) rewards times cumulative log-likelihoods make a far larger inner gradient than the surrogate's, and alpha = 0.1 through
# four steps drives log_std to where exp(-log_std) overflows in the float64 oracle itself under most seeds.  The first seeds from 944 on
# under which the oracle's gradient is finite and meets check_dice_inputs' condition (944: NaN on K_LENGTHS, 1.5e-4 on the seeded case)
DICE_SEEDS = dict(lengths=945, shapes=945)


def dice_cases(K=4, shape='chain'):
    """CPU only -> (check_dice_path_lengths' case on K_LENGTHS, dice_shape_checks' seeded case)"""
    kw = shape_kwargs(shape, K_LENGTHS)
    return (pc.dice_path_lengths_case(DICE_SEEDS['lengths'], K_LENGTHS, O=kw['O'], A=kw['A'], hidden=kw['hidden'], K=K, alpha=ALPHA),
            ds.case(DICE_SEEDS['shapes'], ragged=True, K=K, alpha=ALPHA, **ragged_kwargs(shape)))


def dice_input_figures(c, t64, all_slabs):
    """k_input_figures' second figure for a DiCE case, both outer objectives: by how much of its max-norm the oracle's meta-gradient
    moves under one float32 rounding of the parameters (NaN or inf where the oracle's own chain overflows)"""
    from oracle import dice
    spec = op.PolicySpec(c['O'], c['A'], c['hidden'])
    alpha = np.full(spec.n_params, c['alpha'])
    moved = 0.0
    with np.errstate(all='ignore'):
        for outer in ('dice', 'vpg') if 'vpg_advantages' in all_slabs[c['K']][0] else ('dice',):
            g = dice.meta_objective_and_grad(spec, t64, all_slabs, alpha, outer=outer)['grad']
            if not np.all(np.isfinite(g)):
                return float('nan')
            for draw in range(3):
                off = t64 * (1.0 + 2.0 ** -24 * np.random.RandomState(draw).choice([-1.0, 1.0], t64.size))
                moved = max(moved, pc.rel_max(dice.meta_objective_and_grad(spec, off, all_slabs, alpha, outer=outer)['grad'], g))
    return moved


def check_dice_inputs(K=4, shape='chain'):
    """check_inputs_tell_the_steps_apart's condition (2) on the two DiCE cases"""
    (c, t64, all_slabs), sc_case = dice_cases(K, shape)
    t64s, _, slabs_s = ds.make_case(sc_case)
    for name, moved in (('lengths', dice_input_figures(c, t64, all_slabs)), ('shapes', dice_input_figures(sc_case, t64s, slabs_s))):
        print('count_axes K=%d %s dice %s: the oracle meta-gradient moves by %.2e of its max-norm under one float32 rounding of the '
              'parameters' % (K, shape, name, moved))
        assert moved < 1e-5, (name, moved)


def check_dice_k(lib, K=4, shape='chain'):
    """DICE-MAML's exact gradient through K coupled steps (oracle.dice), then the seeded case of dice_shape_checks: DICE-MAML and
    VPG-DiCE-MAML against oracle.dice and torch.autograd"""
    kw = shape_kwargs(shape, K_LENGTHS)
    sc_case = dice_cases(K, shape)[1]
    worst = {}
    try:
        pc.check_dice_path_lengths(lib, DICE_SEEDS['lengths'], K_LENGTHS, O=kw['O'], A=kw['A'], hidden=kw['hidden'], K=K, alpha=ALPHA, worst=worst)
    finally:
        report('K=%d %s dice' % (K, shape), worst, 'count_axes')
    ds.check_dice_shape(lib, sc_case)
    return worst


@functools.lru_cache(maxsize=None)
def step_size_case(K=4, shape='chain'):
    return sc.PrompCase(k_seed(shape, K), K=K, ragged=True, **ragged_kwargs(shape))


def check_refused_k(lib, K=helpers.ETA_MAX + 1):
    """one step more than PROMP_ETA_MAX: refused by name before anything is allocated"""
    try:
        ctx = _lib.Context(2, 4, 2, (32, 32), K, max_rows=16, max_paths=2, lib=lib)
    except _lib.PrompError as e:
        assert 'num_inner_steps must be in [1, %d]' % helpers.ETA_MAX in str(e), str(e)
    else:
        ctx.close()
        raise AssertionError('num_inner_steps = %d accepted' % K)


@functools.lru_cache(maxsize=None)
def k_input_figures(shape, K, seed=None):
    """CPU only, at check_meta's own inputs -> (the smallest relative difference between two of the oracle's K inner KLs; by how much
    of its max-norm the oracle's meta-gradient moves when every parameter is off by one float32 rounding -- a factor 1 +- 2^-24,
    seeded signs, the largest of three draws)"""
    kw = shape_kwargs(shape, K_LENGTHS)
    seed = k_seed(shape, K) if seed is None else seed
    theta, all_slabs, _ = helpers.make_promp_case(seed, 2, None, None, kw['O'], kw['A'], kw['hidden'], K, lengths_per_task=K_LENGTHS)
    spec = op.PolicySpec(kw['O'], kw['A'], kw['hidden'])
    t64, a64, e64 = theta.astype(np.float64), np.full(spec.n_params, ALPHA), helpers.eta_for(K).astype(np.float64)
    r = pm.meta_objective_and_grad(spec, t64, all_slabs, a64, e64, CLIP)
    kl = np.asarray(r['inner_kl'], np.float64)
    assert kl.shape == (K,) and np.all(kl > 0)
    spread = min(abs(kl[a] - kl[b]) / max(kl[a], kl[b]) for a in range(K) for b in range(a + 1, K))
    moved = 0.0
    for draw in range(3):
        off = t64 * (1.0 + 2.0 ** -24 * np.random.RandomState(draw).choice([-1.0, 1.0], t64.size))
        moved = max(moved, pc.rel_max(pm.meta_objective_and_grad(spec, off, all_slabs, a64, e64, CLIP)['grad'], r['grad']))
    return spread, moved


def check_inputs_tell_the_steps_apart(shape, K):
    """the conditions on the K-axis inputs, oracle alone.  (1) eta and the inner KLs are pairwise different, the KLs by more than
    1e-3 relative: a permuted, truncated or repeated statistics or penalty entry moves the loss by more than ten times its
    tolerance.  (2) The problem can be judged in float32 at all: alpha = 0.1 through eight steps makes the adaptation chain diverge
    under some seeds (inner KLs in the thousands), and there the float64 gradient itself moves by several 1e-5 of its max-norm when
    the parameters are merely rounded to float32 -- such inputs say nothing about a kernel at a tolerance of 1e-4.  The rounding of the
    parameters alone must stay below a tenth of that tolerance.  A seed that fails either is replaced in _K_SEEDS, never the bound."""
    eta = helpers.eta_for(K)
    assert eta.shape == (K,) and len(set(eta.tolist())) == K
    spread, moved = k_input_figures(shape, K)
    print('count_axes K=%d %s: the oracle inner KLs differ pairwise by at least %.2e relative; its meta-gradient moves by %.2e of its '
          'max-norm under one float32 rounding of the parameters' % (K, shape, spread, moved))
    assert spread > 1e-3, (shape, K, spread)
    assert moved < 1e-5, (shape, K, moved)


# ---- M axis ------------------------------------------------------------------------------------------------------------------------
M_TRIPS = (48, 49, 97)               # final_quarter_sum: one full trip; a second holding one task; a third
M_SHAPE = 'chain'


def m_lengths(M, paths=1):
    """every task `paths` paths of 1 .. 20 rows"""
    return [[int(n) for n in row] for row in np.random.RandomState(M).randint(1, 21, size=(M, paths))]


# 900 + M, or the first seed after it under which the inputs meet left_out_sensitivity's condition at that shape (with eight actions
# and a few rows per task the PPO clip sits on every row of a task under most seeds: no gradient from that task)
_M_SEEDS = {(48, 'chain'): 949, (257, 'chain'): 1158, (513, 'layered'): 1414, (257, 'coop_split'): 1204, (513, 'coop_split'): 1451}


def m_seed(M, shape=M_SHAPE):
    return _M_SEEDS.get((M, shape), 900 + M)


def device_cus(lib):
    """the compute units contexts are planned for, PROMP_MAX_CUS unset (256 on the MI355X)"""
    assert not os.environ.get('PROMP_MAX_CUS'), 'PROMP_MAX_CUS is set'
    ctx = _lib.Context(1, 4, 2, (32, 32), 1, max_rows=16, max_paths=1, lib=lib)
    try:
        return int(ctx.device_info()['n_cus'])
    finally:
        ctx.close()


def check_meta_m(lib, M, shape=M_SHAPE, epochs=2):
    return run('M=%d %s meta' % (M, shape), pc.check_meta, lib, m_seed(M, shape), K=1, epochs=epochs, **shape_kwargs(shape, m_lengths(M)))


class TaskCase(sc.PrompCase):
    """step_size_checks.PrompCase on m_lengths(M): what the step-size and the outer-optimiser checks take"""

    def __init__(self, M, shape=M_SHAPE, K=1):
        kw = shape_kwargs(shape, m_lengths(M))
        seed, O, A, hidden = m_seed(M, shape), kw['O'], kw['A'], kw['hidden']
        self.seed, self.M, self.O, self.A, self.hidden, self.K = seed, M, O, A, hidden, K
        self.theta, self.all_slabs, self.all_paths = helpers.make_promp_case(seed, M, None, None, O, A, hidden, K, lengths_per_task=kw['lengths_per_task'])
        self.spec = op.PolicySpec(O, A, hidden)
        self.n = self.spec.n_params
        self.alpha = sc.make_alpha(seed, self.n, A)
        self.eta = helpers.eta_for(K)
        self.coords = sc.fd_coords(seed, self.n, A)
        self.t64, self.a64, self.e64 = self.theta.astype(np.float64), self.alpha.astype(np.float64), self.eta.astype(np.float64)
        self._ref = None


@functools.lru_cache(maxsize=None)
def task_case(M):
    return TaskCase(M)


def check_minibatches_m(lib, M=49, B=3, shape=M_SHAPE):
    """three minibatches over M tasks of three paths each: task i's path p goes to minibatch (i + p) % 3"""
    kw = shape_kwargs(shape, m_lengths(M, paths=B))
    pattern = [(i + p) % B for i in range(M) for p in range(B)]
    mb.check_equals_truncated_batch(lib, m_seed(M), kw['O'], kw['A'], kw['hidden'], 1, lengths=kw['lengths_per_task'], runs=((B, [pattern]),))


@functools.lru_cache(maxsize=None)
def left_out_sensitivity(M, shape=M_SHAPE):
    """CPU only: by how much (of its max-norm) the oracle's meta-gradient moves when one of tasks 0, 47, 48, M - 1 is left out of the
    mean -- the sum runs over the others, the divisor stays M, which is what a final stage that skipped the task would return.
    -> the smallest figure over the four tasks"""
    kw = shape_kwargs(shape, m_lengths(M))
    theta, all_slabs, _ = helpers.make_promp_case(m_seed(M, shape), M, None, None, kw['O'], kw['A'], kw['hidden'], 1, lengths_per_task=kw['lengths_per_task'])
    spec = op.PolicySpec(kw['O'], kw['A'], kw['hidden'])
    t64, a64, e64 = theta.astype(np.float64), np.full(spec.n_params, ALPHA), helpers.eta_for(1).astype(np.float64)
    full = pm.meta_objective_and_grad(spec, t64, all_slabs, a64, e64, CLIP)['grad']
    moved = []
    for i in sorted(set(i for i in (0, 47, 48, M - 1) if i < M)):
        one = pm.meta_objective_and_grad(spec, t64, all_slabs, a64, e64, CLIP, tasks=[i], n_tasks_total=M)['grad']
        moved.append(pc.rel_max(full - one, full))
    return min(moved)


def check_inputs_show_a_left_out_task(M, shape=M_SHAPE):
    """ten times the comparison's tolerance: if a seed does not give it, _M_SEEDS takes another seed, never a smaller bound"""
    moved = left_out_sensitivity(M, shape)
    print('count_axes M=%d %s: the oracle meta-gradient moves by at least %.2e of its max-norm without one of tasks 0, 47, 48, %d'
          % (M, shape, moved, M - 1))
    assert moved >= 1e-3, (M, shape, moved)


# ---- tasks outnumber compute units ---------------------------------------------------------------------------------------------------

def planned_counts(task_rows, n_cus):
    """build_step_tables' counts (promp_plan.h) restated: items of work table 0 and 1, chain segments, chain workgroups, for tasks of
    task_rows rows.  test_count_axes_host.py holds it to the layouts tests/host/plan_check.cpp pins against the C++."""
    tiles = [(int(r) + 15) // 16 for r in task_rows]
    total = sum(tiles)
    items = []
    for t in range(2):
        target = (t + 1) * n_cus
        nw, rem = [], []
        for n in tiles:
            w, r = divmod(n * target, total)
            if w < 1:
                w, r = 1, 0
            if w > n:
                w, r = n, 0
            nw.append(w)
            rem.append(r)
        used = sum(nw)
        while used < target:
            best = -1
            for i in range(len(tiles)):
                if nw[i] < tiles[i] and rem[i] > 0 and (best < 0 or rem[i] > rem[best]):
                    best = i
            if best < 0:
                break
            nw[best] += 1
            rem[best] = 0
            used += 1
        items.append(sum(nw))
    rounds = [(n + 3) // 4 for n in tiles]             # CHAIN_NW_HVP = 4 waves walk a segment's tiles round-robin
    SEGC = 2

    def cut(limit):
        nwg = nseg = cost = 0
        is_open = False
        for r in rounds:
            done = 0
            while done < r:
                room = (limit - cost - SEGC) // 4 if is_open else 0
                if not is_open or room < 1:
                    nwg, is_open, cost = nwg + 1, True, 0
                    room = max((limit - SEGC) // 4, 1)
                take = min(room, r - done)
                nseg += 1
                done += take
                cost += 4 * take + SEGC
        return nwg, nseg
    lo, hi = 4 + SEGC, 4 * sum(rounds) + SEGC * len(tiles) + 4
    while lo < hi:
        mid = (lo + hi) // 2
        if cut(mid)[0] <= n_cus:
            hi = mid
        else:
            lo = mid + 1
    nwg, nseg = cut(lo)
    return dict(items0=items[0], items1=items[1], segments=nseg, workgroups=nwg)


def check_tables_fit(M, n_cus, paths=1):
    """the tables build_step_tables makes of m_lengths(M) stay within max_work = 2 n_cus + M, the size of their device buffers
    (an overflow is refused by name as well: 'internal: work table overflow'); every task is floored to one item when M > n_cus"""
    rows = [sum(lens) for lens in m_lengths(M, paths)]
    c = planned_counts(rows, n_cus)
    max_work = 2 * n_cus + M
    print('count_axes M=%d on %d units: %s, room for %d' % (M, n_cus, '  '.join('%s %d' % kv for kv in sorted(c.items())), max_work))
    assert max(c['items0'], c['items1'], c['segments']) <= max_work and c['workgroups'] <= n_cus, (c, max_work)
    assert min(c['items0'], c['items1'], c['segments']) >= M
    return c


PROC_KWARGS = dict(discount=0.99, gae_lambda=0.97, positive_adv=False)


def check_family_m(lib, shape, M, n_cus):
    """sample processing (k_fit*, k_obs_range, ... on M workgroups) at the shape's obs_dim, then check_meta with one epoch.
    Two paths of 12 rows per task: the fit of a task with fewer rows than feature columns (2 obs_dim + 4) interpolates, and
    normalising advantages of ~1e-8 turns solver noise into O(1) (parity_checks.check_sample_processing_edges), so the advantages are
    normalised only where 24 rows are at least twice the columns."""
    O = K_SHAPES[shape]['O']
    check_tables_fit(M, n_cus)
    pc.check_sample_processing_oracle(lib, m_seed(M), M, 2, 12, O, False, dict(PROC_KWARGS, normalize_adv=24 >= 2 * pc.feature_columns(O, 'linear_feature')))
    return check_meta_m(lib, M, shape, epochs=1)


GOAL_DATA_SEED = {257: 0}            # under which the goal collection of M tasks meets its events and margins (goal_collect_args)


def goal_collect_args(M):
    """one environment per task, max_path_length 3, the wrapped environment, host noise"""
    return dict(M=M, B=1, T=3, hidden=(32, 32), normalization_scale=10, noise='host', step=0, seed=0, clip_infos=True,
                wanted=tuple(e for e in gc.EVENTS if e != 'three_episodes'), data_seed=GOAL_DATA_SEED.get(M, 0))
