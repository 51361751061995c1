"""Checks of the minibatched Adam epochs (promp_optimize_minibatch; MAMLFirstOrderOptimizer's / ProMP's num_minibatches), shared by
test_emu_minibatch.py (emulator, tiny) and test_gpu_minibatch.py (-m gpu).

The core check needs no tolerance.  A minibatch is the meta-objective on fewer paths, and its compact slab is laid out exactly as
an upload of those paths alone would be: a context that holds the whole batch and is told the assignment must leave, bit for bit,
the parameters, Adam slots and trained step sizes that a by-hand sequence leaves -- for every Adam step a FRESH context uploaded
with the minibatch's paths alone (subsample_checks.truncate), given the state so far, doing promp_meta_grad + promp_adam_step.
Any difference is a defect in the copy launch, the tables, the observation ranges it leaves or the sequencing."""
import numpy as np
import pytest

from oracle import policy as op
from oracle import promp as pm
from promp_amd import _lib
from tests import helpers
from tests import subsample_checks as sc
from tests.parity_checks import assert_adam_trajectory, make_ctx

LENGTHS = sc.LENGTHS            # 3 tasks with 5, 3 and 4 paths: [[17, 16, 31, 1, 33], [9, 35, 18], [20, 3, 47, 15]]
# B = 2: task 1 keeps its single 9-row path in share 0
ASSIGN_2 = [0, 1, 0, 1, 1, 0, 1, 1, 1, 0, 0, 1]
ASSIGN_2B = [1, 1, 0, 0, 1, 1, 0, 1, 0, 1, 1, 0]
# B = 3: every share of task 1 is a single path; the 1-row path of task 0 shares with the 16-row one
ASSIGN_3 = [0, 1, 2, 1, 0, 2, 0, 1, 0, 1, 2, 2]
EMU_LENGTHS = sc.EMU_LENGTHS    # [[17, 5, 20], [16, 3]]
EMU_ASSIGN_2 = [0, 1, 0, 1, 0]
LR, CLIP = 1e-3, 0.3


def per_step(base, B, K):
    """one epoch's assignment from a pattern: step k takes the pattern with the minibatches rotated by k (every task still has
    a path in every share, the shares differ from step to step)"""
    return [(np.asarray(base, np.int32) + k) % B for k in range(K + 1)]


def eta_of(K):
    return helpers.eta_for(K)


class Case(object):
    """the whole batch in one context, and what the by-hand sequence needs to rebuild any share of it"""

    def __init__(self, lib, seed, O, A, hidden, K, lengths=LENGTHS, compact_log_std=False, train_sizes=False, alpha=0.05, case=None):
        self.lib, self.O, self.A, self.hidden, self.K, self.M = lib, O, A, hidden, K, len(lengths)
        self.compact_log_std, self.train_sizes = compact_log_std, train_sizes
        self.theta, self.all_slabs, self.all_paths = case if case is not None else sc.make_case(seed, lengths, O, A, hidden, K)
        self.spec = op.PolicySpec(O, A, hidden)
        self.alpha = np.full(self.spec.n_params, alpha, np.float32)
        self.ctx = self.fresh(self.all_paths, self.all_slabs)
        self.reset()

    def fresh(self, paths, slabs):
        ctx = make_ctx(self.lib, self.M, self.O, self.A, self.hidden, self.K, paths)
        helpers.upload_slabs(ctx, paths, slabs, compact_log_std=self.compact_log_std)
        if self.train_sizes:
            ctx.set_train_step_sizes(True)
        return ctx

    def zero_state(self):
        z = np.zeros(self.spec.n_params, np.float32)
        return dict(theta=self.theta.copy(), alpha=self.alpha.copy(), m=z.copy(), v=z.copy(), t=0, sm=z.copy(), sv=z.copy())

    def put(self, ctx, s):
        ctx.set_theta(s['theta'])
        ctx.set_step_sizes(s['alpha'])
        ctx.set_adam_state(s['m'], s['v'], s['t'])
        if self.train_sizes:
            ctx.set_step_size_adam_state(s['sm'], s['sv'])

    def get(self, ctx):
        m, v, t = ctx.get_adam_state()
        s = dict(theta=ctx.get_theta(), alpha=ctx.get_step_sizes(), m=m, v=v, t=t)
        if self.train_sizes:
            s['sm'], s['sv'] = ctx.get_step_size_adam_state()
        return s

    def reset(self):
        self.put(self.ctx, self.zero_state())

    def share(self, epoch, j, slabs=None):
        """(paths, slabs) of minibatch j under one epoch's assignment [K + 1][n_paths]"""
        sels = [np.flatnonzero(np.asarray(a) == j) for a in epoch]
        return sc.truncate(self.all_paths, self.all_slabs if slabs is None else slabs, sels)

    def by_hand(self, assign, B, state, inner_kind, outer_kind=_lib.OUTER_CLIP, slabs=None, eta=None):
        """the Adam steps of `assign` (a list of epochs) one by one, each in a context of its own that holds the share alone"""
        eta = eta_of(self.K) if eta is None else eta
        for epoch in assign:
            for j in range(B):
                ctx = self.fresh(*self.share(epoch, j, slabs))
                self.put(ctx, state)
                ctx.meta_grad(CLIP, eta, inner_kind=inner_kind, outer_kind=outer_kind)
                ctx.adam_step(LR)
                state = self.get(ctx)
                ctx.close()
        return state

    def close(self):
        self.ctx.close()


def same_state(a, b):
    assert a['t'] == b['t'], (a['t'], b['t'])
    for k in a:
        if k != 't':
            assert np.array_equal(a[k], b[k]), (k, float(np.max(np.abs(a[k].astype(np.float64) - b[k]))))


def check_equals_truncated_batch(lib, seed, O, A, hidden, K, inner='loglik', compact_log_std=False, train_sizes=False, lengths=LENGTHS,
                                 runs=None):
    """item 2.  runs: (B, [pattern per epoch]); the default is B = 2 and B = 3 with one epoch each, then two epochs of B = 2 with
    different assignments -- the by-hand sequence of the second continues the first one's"""
    kind = dict(loglik=_lib.INNER_LOGLIK, ratio=_lib.INNER_RATIO)[inner]
    c = Case(lib, seed, O, A, hidden, K, lengths=lengths, compact_log_std=compact_log_std, train_sizes=train_sizes)
    eta = eta_of(K)
    if runs is None:
        runs = ((2, [ASSIGN_2]), (3, [ASSIGN_3]), (2, [ASSIGN_2, ASSIGN_2B]))
    hand = {}
    for B, patterns in runs:
        assign = [per_step(p, B, K) for p in patterns]
        c.reset()
        r = c.ctx.optimize_minibatch(len(assign), B, assign, LR, CLIP, eta, inner_kind=kind)
        got = c.get(c.ctx)
        assert got['t'] == B * len(assign) and np.isfinite(got['theta']).all() and np.isfinite(r['loss_after'])
        # (an epoch whose predecessors were walked by hand already: go on from there)
        key = (B, tuple(tuple(p) for p in patterns[:-1]))
        start = hand.get(key, None) if len(patterns) > 1 else None
        want = c.by_hand(assign[-1:] if start else assign, B, start or c.zero_state(), kind)
        hand[(B, tuple(tuple(p) for p in patterns))] = want
        same_state(got, want)
        assert not np.array_equal(got['theta'], c.theta)
        if train_sizes:
            assert not np.array_equal(got['alpha'], c.alpha)
    c.close()


def check_one_minibatch_is_optimize(lib, seed, O, A, hidden, K=1, epochs=2):
    """item 3: B = 1 is today's call, from the same state (an inner_adapt in front: the first epoch takes its pass over)"""
    eta = eta_of(K)
    out = []
    for call in ('optimize', 'minibatch'):
        c = Case(lib, seed, O, A, hidden, K)
        c.ctx.switch_to_pre_update()
        c.ctx.inner_adapt(0)
        skipped = c.ctx.adapt_passes_skipped()
        if call == 'optimize':
            r = c.ctx.optimize(epochs, LR, CLIP, eta)
        else:
            r = c.ctx.optimize_minibatch(epochs, 1, None, LR, CLIP, eta)
        out.append((c.get(c.ctx), r, c.ctx.adapt_passes_skipped() - skipped))
        c.close()
    (s0, r0, k0), (s1, r1, k1) = out
    same_state(s0, s1)
    assert k0 == k1 == 1
    assert r0['loss_before'] == r1['loss_before'] and r0['loss_after'] == r1['loss_after'] and r0['outer_kl'] == r1['outer_kl']
    assert np.array_equal(r0['inner_kl'], r1['inner_kl'])


def check_python_path_one_minibatch(lib, seed, O, A, hidden, K=1, T=20, epochs=2):
    """item 3, the Python path: ProMP(num_minibatches=1) is ProMP as it was -- the parameters and statistics of optimize()"""
    from promp_amd import session
    from promp_amd.utils import logger
    logger.configure(quiet=True)
    M, P = 3, 4
    case = helpers.make_promp_case(seed, M, P, T, O, A, hidden, K)
    theta, all_slabs, _ = case
    _lib.set_library_for_testing(lib)
    try:
        algo, policy, samples = _promp(lib, theta, all_slabs, M, P, O, A, hidden, K, num_ppo_steps=epochs, num_minibatches=1)
        algo.optimize_policy(samples, log=False)
        got, stats = _flat(policy), algo.last_stats
    finally:
        _lib.set_library_for_testing(None)
        session._current = None
    c = Case(lib, seed, O, A, hidden, K, lengths=[[T] * P] * M, case=case)
    r = c.ctx.optimize(epochs, LR, CLIP, eta_of(1)[0] * np.ones(K, np.float32))
    assert np.array_equal(got, c.ctx.get_theta())
    for k in ('loss_before', 'loss_after', 'outer_kl', 'inner_kl'):
        assert np.array_equal(stats[k], r[k]), k
    c.close()


def check_statistics(lib, seed, O=5, A=3, hidden=(32, 32), K=1, lengths=LENGTHS, pattern=ASSIGN_2):
    """item 4: loss_before and the statistics behind the last step are the whole batch's"""
    c = Case(lib, seed, O, A, hidden, K, lengths=lengths)
    eta = eta_of(K)
    before = c.ctx.meta_eval(CLIP, eta)
    r = c.ctx.optimize_minibatch(1, 2, [per_step(pattern, 2, K)], LR, CLIP, eta)
    after = c.ctx.meta_eval(CLIP, eta)
    assert r['loss_before'] == before['loss']
    assert r['loss_after'] == after['loss'] and r['outer_kl'] == after['outer_kl'] and np.array_equal(r['inner_kl'], after['inner_kl'])
    assert r['loss_after'] != r['loss_before']
    c.close()


def check_against_float64(lib, seed, O, A, hidden, K, lengths=LENGTHS, patterns=(ASSIGN_2, ASSIGN_2B)):
    """item 5: the parameters after 1 and after 2 epochs of B = 2 against the float64 sequence assembled from the oracle's
    meta_objective_and_grad and adam_step on the truncated slabs, with the rule and the constants of the small-case
    Adam-trajectory comparison at these shapes: parity_checks.assert_adam_trajectory as check_meta applies it
    (tests/parity_checks.py:598; ADAM_GRAD_FLOOR, ADAM_STEP_TOL, ADAM_MAX_EXCLUDED at :496-498)"""
    B = 2
    c = Case(lib, seed, O, A, hidden, K, lengths=lengths, alpha=0.1)
    eta = eta_of(K)
    a64, e64, t64 = c.alpha.astype(np.float64), eta.astype(np.float64), c.theta.astype(np.float64)
    assign = [per_step(p, B, K) for p in patterns]
    th, st, gmin, gmax = t64.copy(), pm.AdamState(c.spec.n_params), None, []
    worst = []
    for e, epoch in enumerate(assign):
        for j in range(B):
            _, sub = c.share(epoch, j)
            g = pm.meta_objective_and_grad(c.spec, th, sub, a64, e64, CLIP)['grad']
            gmin = np.abs(g) if gmin is None else np.minimum(gmin, np.abs(g))
            gmax.append(np.max(np.abs(g)))
            th = pm.adam_step(th, g, st, LR)
        c.reset()
        c.ctx.optimize_minibatch(e + 1, B, assign[:e + 1], LR, CLIP, eta)
        got = c.get(c.ctx)
        assert got['t'] == B * (e + 1)
        worst.append(assert_adam_trajectory(got['theta'].astype(np.float64) - t64, th - t64, gmin, np.array(gmax), LR, B * (e + 1),
                                            m_dev=got['m'], v_dev=got['v'], m_ref=st.m, v_ref=st.v))
    print('minibatch trajectory vs float64 (fraction of lr, excluded share) per epoch:', worst)
    c.close()


def check_state_left_behind(lib, seed, O=5, A=3, hidden=(32, 32), K=1, lengths=LENGTHS, pattern=ASSIGN_2, selections=sc.SELECTIONS):
    """item 6"""
    eta = eta_of(K)
    assign = [per_step(pattern, 2, K)]
    c = Case(lib, seed, O, A, hidden, K, lengths=lengths)
    v = np.random.RandomState(seed + 1).randn(c.spec.n_params).astype(np.float32)
    # a TRPO selection set beforehand evaluates to the same bits afterwards
    for k in range(K + 1):
        c.ctx.set_step_selection(k, selections[k % len(selections)])
    c.ctx.use_selection(True)
    h0 = c.ctx.constraint_hvp(v, inner_kind=_lib.INNER_LOGLIK, refresh_chain=True)
    c.ctx.optimize_minibatch(1, 2, assign, LR, CLIP, eta)
    first = c.get(c.ctx)
    c.reset()
    assert np.array_equal(c.ctx.constraint_hvp(v, inner_kind=_lib.INNER_LOGLIK, refresh_chain=True), h0)
    c.ctx.use_selection(False)
    c.ctx.clear_selections()
    # inner_adapt + a B = 1 optimise: the bits of a fresh context
    out = []
    for ctx in (c.ctx, c.fresh(c.all_paths, c.all_slabs)):
        c.put(ctx, c.zero_state())
        ctx.switch_to_pre_update()
        ctx.inner_adapt(0)
        r = ctx.optimize_minibatch(2, 1, None, LR, CLIP, eta)
        out.append((c.get(ctx), r))
    same_state(out[0][0], out[1][0])
    assert out[0][1]['loss_before'] == out[1][1]['loss_before'] and out[0][1]['loss_after'] == out[1][1]['loss_after']
    out[1] = None
    ctx.close()
    # new data between two minibatched calls is seen
    rng = np.random.RandomState(seed + 2)
    new_slabs = [[dict(s, advantages=rng.randn(len(s['advantages'])).astype(np.float32)) for s in slabs] for slabs in c.all_slabs]
    for k in range(K + 1):
        c.ctx.set_advantages(k, np.concatenate([s['advantages'] for s in new_slabs[k]]))
    c.reset()
    c.ctx.optimize_minibatch(1, 2, assign, LR, CLIP, eta)
    second = c.get(c.ctx)
    assert not np.array_equal(second['theta'], first['theta'])
    other = c.fresh(c.all_paths, new_slabs)
    c.put(other, c.zero_state())
    other.optimize_minibatch(1, 2, assign, LR, CLIP, eta)
    same_state(second, c.get(other))
    other.close()
    c.close()


def check_refusals(lib, seed=5, O=5, A=3, hidden=(32, 32), K=1, lengths=LENGTHS, pattern=ASSIGN_2):
    """item 7 (library level): each refusal names its reason and moves nothing"""
    c = Case(lib, seed, O, A, hidden, K, lengths=lengths)
    eta = eta_of(K)
    n = len(pattern)
    good = per_step(pattern, 2, K)
    before, ver = c.get(c.ctx), c.ctx.state_version()

    def refused(msg, call):
        with pytest.raises(_lib.PrompError, match=msg):
            call()
        same_state(c.get(c.ctx), before)
        assert c.ctx.state_version() == ver

    bad = [a.copy() for a in good]
    bad[K][3] = 2
    refused('epoch 0, step %d.*minibatch 2 out of range' % K, lambda: c.ctx.optimize_minibatch(1, 2, [bad], LR, CLIP, eta))
    bad = [a.copy() for a in good]
    bad[0][3] = -1
    refused('minibatch -1 out of range', lambda: c.ctx.optimize_minibatch(1, 2, [bad], LR, CLIP, eta))
    # the second epoch is checked before the first one is enqueued
    empty = [a.copy() for a in good]
    task1 = slice(len(lengths[0]), len(lengths[0]) + len(lengths[1]))
    empty[0][task1] = 1
    refused('epoch 1, step 0.*leaves minibatch 0 without a path of task 1',
            lambda: c.ctx.optimize_minibatch(2, 2, [good, empty], LR, CLIP, eta))
    fewest = min(len(l) for l in lengths)
    refused('exceeds the %d paths' % fewest,
            lambda: c.ctx.optimize_minibatch(1, fewest + 1, [[np.zeros(n, np.int32)] * (K + 1)], LR, CLIP, eta))
    refused('below 1', lambda: c.ctx.optimize_minibatch(1, 0, [good], LR, CLIP, eta))
    refused('entries', lambda: c.ctx.optimize_minibatch(1, 2, [[good[0][:-1]] + good[1:]], LR, CLIP, eta))
    refused('DiCE', lambda: c.ctx.optimize_minibatch(1, 2, [good], LR, CLIP, eta, inner_kind=_lib.INNER_DICE))
    # a pending optimisation (of no epochs: it moves nothing either)
    c.ctx.optimize_begin(0, LR, CLIP, eta)
    refused('has not been collected', lambda: c.ctx.optimize_minibatch(1, 2, [good], LR, CLIP, eta))
    refused('has not been collected', lambda: c.ctx.optimize_minibatch(1, 1, None, LR, CLIP, eta))
    c.ctx.optimize_end()
    same_state(c.get(c.ctx), before)
    # and afterwards the call goes through
    c.ctx.optimize_minibatch(1, 2, [good], LR, CLIP, eta)
    assert c.get(c.ctx)['t'] == 2
    # a step that carries DiCE rewards is not dealt to minibatches, whatever the inner kind
    c.ctx.set_dice_rewards(0, np.ones(sum(lengths[i][p] for i in range(len(lengths)) for p in range(len(lengths[i]))), np.float32))
    before, ver = c.get(c.ctx), c.ctx.state_version()
    refused('step 0 carries DiCE rewards', lambda: c.ctx.optimize_minibatch(1, 2, [good], LR, CLIP, eta))
    c.close()


# ---- plugin level -----------------------------------------------------------------------------------------------------------

def _promp(lib, theta, all_slabs, M, P, O, A, hidden, K, **kw):
    from promp_amd.meta_algos.pro_mp import ProMP
    from promp_amd.policies.meta_gaussian_mlp_policy import MetaGaussianMLPPolicy
    spec = op.PolicySpec(O, A, hidden)
    policy = MetaGaussianMLPPolicy(name='p', obs_dim=O, action_dim=A, meta_batch_size=M, hidden_sizes=hidden)
    policy.set_params(spec.to_ordered_dict(theta))
    algo = ProMP(policy=policy, inner_lr=0.05, meta_batch_size=M, num_inner_grad_steps=K, learning_rate=LR, clip_eps=CLIP,
                 init_inner_kl_penalty=float(eta_of(1)[0]), adaptive_inner_kl_penalty=False, **kw)
    samples = [[dict(observations=d['observations'], actions=d['actions'], advantages=d['advantages'], agent_infos=d['agent_infos'],
                     path_lengths=[len(d['advantages']) // P] * P) for d in step] for step in all_slabs]
    return algo, policy, samples


def _flat(policy):
    return np.concatenate([np.asarray(v, np.float32).reshape(-1) for v in policy.get_param_values().values()])


def check_plugin(lib, seed, O=5, A=3, hidden=(32, 32), K=1, T=20, draw_seed=4321):
    """item 8: ProMP(num_minibatches=2, num_ppo_steps=2) against the by-hand sequence on the assignments minibatch_assignment draws
    under the same seed; it is not what num_minibatches=1 gives; external-collective mode refuses"""
    from promp_amd import session
    from promp_amd.optimizers.maml_first_order_optimizer import minibatch_assignment
    from promp_amd.utils import logger
    logger.configure(quiet=True)
    M, P, E, B = 3, 4, 2, 2
    case = helpers.make_promp_case(seed, M, P, T, O, A, hidden, K)
    theta, all_slabs, _ = case
    _lib.set_library_for_testing(lib)
    try:
        thetas = {}
        for nb in (B, 1):
            algo, policy, samples = _promp(lib, theta, all_slabs, M, P, O, A, hidden, K, num_ppo_steps=E, num_minibatches=nb)
            np.random.seed(draw_seed)
            algo.optimize_policy(samples, log=False)
            thetas[nb] = _flat(policy)
            stats = algo.last_stats
            assert algo.optimizer.last_result is stats and np.isfinite(stats['loss_before']) and np.isfinite(stats['loss_after'])
            # compute_stats behind optimize answers from what the call handed back
            assert algo.optimizer.compute_stats(dict(clip_eps=algo.clip_eps, inner_kl_coeff=algo.inner_kl_coeff))[0] == stats['loss_after']
            if nb == B:
                # external-collective mode: refused with the reason, nothing moved
                s = algo.session
                ver, th = s.ctx.state_version(), s.ctx.get_theta()
                s.world, s.collective = 2, (lambda values, op_: values)
                with pytest.raises(_lib.PrompError, match='external collective'):
                    algo.optimizer.optimize()
                with pytest.raises(_lib.PrompError, match='external collective'):
                    s.optimize(E, LR, CLIP, algo.inner_kl_coeff, num_minibatches=B, assign=None)
                s.world, s.collective = 1, None
                assert s.ctx.state_version() == ver and np.array_equal(s.ctx.get_theta(), th)
            session._current = None
        np.random.seed(draw_seed)
        assign = [[minibatch_assignment([P] * M, B) for _ in range(K + 1)] for _ in range(E)]
        c = Case(lib, seed, O, A, hidden, K, lengths=[[T] * P] * M, case=case)
        eta = eta_of(1)[0] * np.ones(K, np.float32)
        state = c.by_hand(assign, B, c.zero_state(), _lib.INNER_RATIO, eta=eta)
        c.close()
        assert np.array_equal(thetas[B], state['theta'])
        # fails without the feature: the argument is no longer ignored
        assert not np.array_equal(thetas[B], thetas[1])
    finally:
        _lib.set_library_for_testing(None)
        session._current = None
