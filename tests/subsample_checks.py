"""Checks of the subsampled constraint products (promp_set_step_selection, promp_use_selection; ConjugateGradientOptimizer's
subsample_factor), shared by test_emu_subsample.py (emulator, tiny) and test_gpu_subsample.py (-m gpu).

The core check needs no tolerance: a context that holds the whole batch plus a selection (A) must compute, bit for bit, what a
context created for and uploaded with the selected paths alone (B) computes -- the compact slab is laid out exactly as that
upload would lay it out, so any difference is a defect in the gather, the tables or the sequencing."""
from collections import OrderedDict

import numpy as np
import pytest

from oracle import policy as op
from oracle import promp as pm
from promp_amd import _lib
from tests import helpers
from tests.parity_checks import make_ctx, on_policy_case, rel_max

# 3 tasks with 5, 3 and 4 paths; ragged lengths, none a multiple of 16 but one
LENGTHS = [[17, 16, 31, 1, 33], [9, 35, 18], [20, 3, 47, 15]]
# per step (cycled): one path left in task 1, the first path of tasks 0 and 2 dropped, the last path of the last task dropped
SELECTIONS = [[1, 3, 4, 6, 9, 10], [0, 2, 5, 7, 8, 10], [1, 2, 3, 4, 5, 6, 7, 9, 10]]
EMU_LENGTHS = [[17, 5, 20], [16, 3]]
EMU_SELECTIONS = [[1, 2, 4], [0, 2, 3]]


def make_case(seed, lengths, O, A, hidden, K):
    """slabs and paths of steps 0..K with the given path lengths per task (the recipe of helpers.make_promp_case)"""
    from promp_amd import synthetic
    rng = np.random.RandomState(seed)
    theta = synthetic.init_theta(rng, O, hidden, A)
    theta = (theta + 0.05 * rng.randn(theta.size)).astype(np.float32)
    all_slabs, all_paths = [], []
    for k in range(K + 1):
        old = (theta + 0.1 * rng.randn(theta.size)).astype(np.float32)
        paths = helpers.make_paths_with_lengths(rng, old[None, :], lengths, O, A, hidden)
        slabs = []
        for plist in paths.values():
            cat = lambda key: np.concatenate([p[key] for p in plist])
            slabs.append(dict(observations=cat('observations'), actions=cat('actions'),
                              advantages=rng.randn(len(cat('rewards'))).astype(np.float32),
                              agent_infos=dict(mean=np.concatenate([p['agent_infos']['mean'] for p in plist]),
                                               log_std=np.concatenate([p['agent_infos']['log_std'] for p in plist]))))
        all_slabs.append(slabs)
        all_paths.append(paths)
    return theta, all_slabs, all_paths


def truncate(all_paths, all_slabs, selections):
    """the batch of the selected paths alone: what context B is uploaded with (selections[k]: flat path indices of step k)"""
    out_paths, out_slabs = [], []
    for paths, slabs, sel in zip(all_paths, all_slabs, selections):
        sel = set(int(j) for j in sel)
        tp, ts, flat = OrderedDict(), [], 0
        for (task, plist), slab in zip(paths.items(), slabs):
            keep_paths, rows, r = [], [], 0
            for p in plist:
                n = len(p['rewards'])
                if flat in sel:
                    keep_paths.append(p)
                    rows.extend(range(r, r + n))
                r += n
                flat += 1
            rows = np.asarray(rows, dtype=np.int64)
            tp[task] = keep_paths
            ts.append(dict(observations=slab['observations'][rows], actions=slab['actions'][rows], advantages=slab['advantages'][rows],
                           agent_infos=dict(mean=slab['agent_infos']['mean'][rows], log_std=slab['agent_infos']['log_std'][rows])))
        out_paths.append(tp)
        out_slabs.append(ts)
    return out_paths, out_slabs


def _pair(lib, seed, lengths, selections, O, A, hidden, K, compact_log_std=False, alpha_value=0.05):
    theta, all_slabs, all_paths = make_case(seed, lengths, O, A, hidden, K)
    sels = [selections[k % len(selections)] for k in range(K + 1)]
    sub_paths, sub_slabs = truncate(all_paths, all_slabs, sels)
    spec = op.PolicySpec(O, A, hidden)
    alpha = np.full(spec.n_params, alpha_value, np.float32)
    M = len(lengths)
    ctxs = []
    for paths, slabs in ((all_paths, all_slabs), (sub_paths, sub_slabs)):
        ctx = make_ctx(lib, M, O, A, hidden, K, paths)
        helpers.upload_slabs(ctx, paths, slabs, compact_log_std=compact_log_std)
        ctx.set_theta(theta)
        ctx.set_step_sizes(alpha)
        ctxs.append(ctx)
    return ctxs[0], ctxs[1], sels, dict(theta=theta, alpha=alpha, spec=spec, all_slabs=all_slabs, sub_slabs=sub_slabs, all_paths=all_paths)


def _select(ctx, sels):
    for k, s in enumerate(sels):
        ctx.set_step_selection(k, s)


def check_equals_truncated_batch(lib, seed, O, A, hidden, K, inner='loglik', compact_log_std=False, lengths=LENGTHS,
                                 selections=SELECTIONS, solves=((0, 2), (1, 2), (2, 3))):
    """item 1: constraint gradient, exact product (refreshed, then not), cg_solve per (mode, iterations) in `solves`; and what A
    holds afterwards"""
    kind = dict(loglik=_lib.INNER_LOGLIK, ratio=_lib.INNER_RATIO)[inner]
    A_, B_, sels, c = _pair(lib, seed, lengths, selections, O, A, hidden, K, compact_log_std)
    eta = np.zeros(K, np.float32)
    rng = np.random.RandomState(seed + 7)
    v = rng.randn(c['spec'].n_params).astype(np.float32)
    A_.switch_to_pre_update()
    A_.inner_adapt(0, inner_kind=kind)           # leaves the first inner pass behind (adapt0): a selection must not take it for its own
    before_g, before_st = A_.meta_grad(0.0, eta, inner_kind=kind, outer_kind=_lib.OUTER_RATIO)
    before_h = A_.constraint_hvp(v, inner_kind=kind, refresh_chain=True)
    _select(A_, sels)
    assert [A_.step_selection(k) for k in range(K + 1)] == [len(s) for s in sels]
    A_.use_selection(True)
    gA = A_.meta_grad(0.0, eta, inner_kind=kind, outer_kind=_lib.OUTER_KL)
    gB = B_.meta_grad(0.0, eta, inner_kind=kind, outer_kind=_lib.OUTER_KL)
    assert np.array_equal(gA[0], gB[0]) and gA[1]['outer_kl'] == gB[1]['outer_kl']
    for refresh in (True, False):
        assert np.array_equal(A_.constraint_hvp(v, inner_kind=kind, refresh_chain=refresh),
                              B_.constraint_hvp(v, inner_kind=kind, refresh_chain=refresh)), refresh
    # the loss gradient is the whole batch's whatever the switch says
    g_mid, _ = A_.meta_grad(0.0, eta, inner_kind=kind, outer_kind=_lib.OUTER_RATIO)
    assert np.array_equal(g_mid, before_g)
    A_.use_selection(False)
    for mode, iters in solves:
        xa, qa = A_.cg_solve(before_g, cg_iters=iters, hvp_mode=mode, inner_kind=kind)
        xb, qb = B_.cg_solve(before_g, cg_iters=iters, hvp_mode=mode, inner_kind=kind)
        assert np.array_equal(xa, xb) and qa == qb, (mode, rel_max(xa, xb.astype(np.float64)), qa, qb)
        assert np.isfinite(xa).all() and np.isfinite(qa)
    # afterwards in A
    after_g, after_st = A_.meta_grad(0.0, eta, inner_kind=kind, outer_kind=_lib.OUTER_RATIO)
    assert np.array_equal(after_g, before_g) and after_st['loss'] == before_st['loss'] and after_st['outer_kl'] == before_st['outer_kl']
    assert np.array_equal(A_.get_theta(), c['theta'])
    A_.clear_selections()
    assert [A_.step_selection(k) for k in range(K + 1)] == [0] * (K + 1)
    assert np.array_equal(A_.constraint_hvp(v, inner_kind=kind, refresh_chain=True), before_h)
    A_.close()
    B_.close()


def check_full_selection_is_no_selection(lib, seed, O, A, hidden, K, lengths=LENGTHS, solves=((0, 2), (2, 2))):
    """item 2: every path selected = no selection, bit for bit"""
    theta, all_slabs, all_paths = make_case(seed, lengths, O, A, hidden, K)
    spec = op.PolicySpec(O, A, hidden)
    n_paths = sum(len(l) for l in lengths)
    eta = np.zeros(K, np.float32)
    v = np.random.RandomState(seed + 3).randn(spec.n_params).astype(np.float32)
    out = []
    for select in (False, True):
        ctx = make_ctx(lib, len(lengths), O, A, hidden, K, all_paths)
        helpers.upload_slabs(ctx, all_paths, all_slabs)
        ctx.set_theta(theta)
        ctx.set_step_sizes(np.full(spec.n_params, 0.05, np.float32))
        b = ctx.meta_grad(0.0, eta, inner_kind=_lib.INNER_LOGLIK, outer_kind=_lib.OUTER_RATIO)[0]
        if select:
            _select(ctx, [list(range(n_paths))] * (K + 1))
            ctx.use_selection(True)
        r = [ctx.meta_grad(0.0, eta, inner_kind=_lib.INNER_LOGLIK, outer_kind=_lib.OUTER_KL)[0],
             ctx.constraint_hvp(v, inner_kind=_lib.INNER_LOGLIK, refresh_chain=True)]
        for mode, iters in solves:
            x, q = ctx.cg_solve(b, cg_iters=iters, hvp_mode=mode, inner_kind=_lib.INNER_LOGLIK)
            r += [x, np.float64(q)]
        out.append(r)
        ctx.close()
    for x, y in zip(*out):
        assert np.array_equal(x, y)


def check_oracle(lib, seed, O, A, hidden, K, lengths=LENGTHS, selections=SELECTIONS):
    """item 3: the constraint gradient on a selection against the float64 oracle's gradient of the KL outer objective on the
    truncated slabs (the function oracle/trpo.py:constraint_hvp_fd64 differences), to the meta-gradient parity checks' 1e-4 of
    the max-norm (parity_checks.check_meta); the exact product on a selection: x.Hx > 0, symmetric to 1e-3"""
    A_, B_, sels, c = _pair(lib, seed, lengths, selections, O, A, hidden, K)
    B_.close()
    spec, eta = c['spec'], np.zeros(K, np.float32)
    _select(A_, sels)
    A_.use_selection(True)
    g, st = A_.meta_grad(0.0, eta, inner_kind=_lib.INNER_LOGLIK, outer_kind=_lib.OUTER_KL)
    r = pm.meta_objective_and_grad(spec, c['theta'].astype(np.float64), c['sub_slabs'], c['alpha'].astype(np.float64), np.zeros(K), 0.0,
                                   pm.INNER_LOGLIK, 'kl', want_grad=True)
    assert rel_max(g, r['grad']) < 1e-4, rel_max(g, r['grad'])
    np.testing.assert_allclose(st['outer_kl'], r['outer_kl'], rtol=1e-4)
    # ... and it is not the whole batch's
    full = pm.meta_objective_and_grad(spec, c['theta'].astype(np.float64), c['all_slabs'], c['alpha'].astype(np.float64), np.zeros(K), 0.0,
                                      pm.INNER_LOGLIK, 'kl', want_grad=True)
    assert rel_max(g, full['grad']) > 1e-2
    rng = np.random.RandomState(seed + 1)
    x, y = rng.randn(spec.n_params).astype(np.float32), rng.randn(spec.n_params).astype(np.float32)
    hx = A_.constraint_hvp(x, inner_kind=_lib.INNER_LOGLIK, refresh_chain=True)
    hy = A_.constraint_hvp(y, inner_kind=_lib.INNER_LOGLIK, refresh_chain=False)
    assert float(np.dot(x, hx)) > 0 and float(np.dot(y, hy)) > 0
    a, b = float(np.dot(y, hx)), float(np.dot(x, hy))
    assert abs(a - b) <= 1e-3 * max(abs(a), abs(b)), (a, b)
    A_.close()


def _check_resizing(lib, seed, O, A, hidden, K, lengths, selections, solves):
    """one context, three selections in turn -- one, a larger one (the compact slab's buffers and its primal cache grow), a smaller
    one (rows of the larger one stay behind the slab's end): each solve is, bit for bit, the solve of a fresh context that holds
    the selected paths alone"""
    theta, all_slabs, all_paths = make_case(seed, lengths, O, A, hidden, K)
    spec = op.PolicySpec(O, A, hidden)
    alpha = np.full(spec.n_params, 0.05, np.float32)
    b = np.random.RandomState(seed + 9).randn(spec.n_params).astype(np.float32)
    M = len(lengths)
    last = np.cumsum([len(l) for l in lengths]) - 1
    first, larger, smaller = list(selections[0]), sorted(set(selections[0]) | set(selections[1])), [int(p) for p in last]
    assert len(smaller) < len(first) < len(larger)

    def ctx_of(paths, slabs):
        ctx = make_ctx(lib, M, O, A, hidden, K, paths)
        helpers.upload_slabs(ctx, paths, slabs)
        ctx.set_theta(theta)
        ctx.set_step_sizes(alpha)
        return ctx

    A_ = ctx_of(all_paths, all_slabs)
    for sel in (first, larger, smaller):
        sels = [sel] * (K + 1)
        B_ = ctx_of(*truncate(all_paths, all_slabs, sels))
        _select(A_, sels)
        for mode, iters in solves:
            xa, qa = A_.cg_solve(b, cg_iters=iters, hvp_mode=mode, inner_kind=_lib.INNER_LOGLIK)
            xb, qb = B_.cg_solve(b, cg_iters=iters, hvp_mode=mode, inner_kind=_lib.INNER_LOGLIK)
            assert np.array_equal(xa, xb) and qa == qb, (len(sel), mode, rel_max(xa, xb.astype(np.float64)), qa, qb)
            assert np.isfinite(xa).all() and np.isfinite(qa)
        B_.close()
    A_.close()


def check_staleness(lib, seed, O=5, A=3, hidden=(32, 32), K=1, lengths=LENGTHS, selections=SELECTIONS, resize_solves=((2, 2), (0, 1))):
    """item 4; and a selection replaced by a larger, then by a smaller one"""
    _check_resizing(lib, seed + 20, O, A, hidden, K, lengths, selections, resize_solves)
    A_, B_, sels, c = _pair(lib, seed, lengths, selections, O, A, hidden, K)
    kind, eta = _lib.INNER_LOGLIK, np.zeros(K, np.float32)
    v = np.random.RandomState(seed + 5).randn(c['spec'].n_params).astype(np.float32)
    _select(A_, sels)
    A_.use_selection(True)
    h0 = A_.constraint_hvp(v, inner_kind=kind, refresh_chain=True)
    # new advantages after the selection are seen by the next product
    rng = np.random.RandomState(seed + 6)
    new_slabs = [[dict(s, advantages=rng.randn(len(s['advantages'])).astype(np.float32)) for s in slabs] for slabs in c['all_slabs']]
    _, new_sub = truncate(c['all_paths'], new_slabs, sels)
    for k in range(K + 1):
        A_.set_advantages(k, np.concatenate([s['advantages'] for s in new_slabs[k]]))
        B_.set_advantages(k, np.concatenate([s['advantages'] for s in new_sub[k]]))
    h1 = A_.constraint_hvp(v, inner_kind=kind, refresh_chain=True)
    assert np.array_equal(h1, B_.constraint_hvp(v, inner_kind=kind, refresh_chain=True))
    assert not np.array_equal(h1, h0)
    b = A_.meta_grad(0.0, eta, inner_kind=kind, outer_kind=_lib.OUTER_RATIO)[0]
    # DiCE on a selection is refused; the refusal moves nothing
    ver = A_.state_version()
    with pytest.raises(_lib.PrompError, match='DiCE'):
        A_.cg_solve(b, cg_iters=1, hvp_mode=2, inner_kind=_lib.INNER_DICE)
    with pytest.raises(_lib.PrompError, match='DiCE'):
        A_.meta_grad(0.0, eta, inner_kind=_lib.INNER_DICE, outer_kind=_lib.OUTER_KL)
    assert A_.state_version() == ver
    # a new upload clears the step's selection; a solve with selections on some steps only is refused
    fl = _lib.flatten_paths(c['all_paths'][0])
    A_.upload_step(0, fl['task_path_offsets'], fl['path_row_offsets'], fl['obs'], fl['rew'], fl['act'], fl['old_mean'], fl['old_log_std'])
    A_.set_advantages(0, np.concatenate([s['advantages'] for s in new_slabs[0]]))
    assert A_.step_selection(0) == 0 and A_.step_selection(K) == len(sels[K])
    ver, th = A_.state_version(), A_.get_theta()
    for call in (lambda: A_.cg_solve(b, cg_iters=1, hvp_mode=0, inner_kind=kind),
                 lambda: A_.cg_solve(b, cg_iters=1, hvp_mode=2, inner_kind=kind),
                 lambda: A_.constraint_hvp(v, inner_kind=kind, refresh_chain=True),
                 lambda: A_.meta_grad(0.0, eta, inner_kind=kind, outer_kind=_lib.OUTER_KL)):
        with pytest.raises(_lib.PrompError, match='of %d steps have a selection' % (K + 1)):
            call()
    assert A_.state_version() == ver and np.array_equal(A_.get_theta(), th)
    # selected again: the same bits as before the upload (same data)
    A_.set_step_selection(0, sels[0])
    assert np.array_equal(A_.constraint_hvp(v, inner_kind=kind, refresh_chain=True), h1)
    A_.close()
    B_.close()


def check_malformed(lib, seed=3, O=5, A=3, hidden=(32, 32), K=1, lengths=LENGTHS):
    """item 5: refused with a message, and nothing written: the selection that stood still stands, bit for bit"""
    theta, all_slabs, all_paths = make_case(seed, lengths, O, A, hidden, K)
    spec = op.PolicySpec(O, A, hidden)
    ctx = make_ctx(lib, len(lengths), O, A, hidden, K, all_paths)
    helpers.upload_slabs(ctx, all_paths, all_slabs)
    ctx.set_theta(theta)
    ctx.set_step_sizes(np.full(spec.n_params, 0.05, np.float32))
    good = SELECTIONS[0]
    _select(ctx, [good] * (K + 1))
    ctx.use_selection(True)
    v = np.random.RandomState(seed).randn(spec.n_params).astype(np.float32)
    h = ctx.constraint_hvp(v, refresh_chain=True)
    ver = ctx.state_version()
    n = sum(len(l) for l in lengths)
    for bad, msg in (([1, 4, 3, 6, 9, 10], 'not sorted'), ([1, 3, 3, 6, 9, 10], 'repeats path 3'), ([1, 3, 6, 9, n], 'out of range'),
                     ([-1, 3, 6, 9], 'out of range'), ([0, 1, 2, 3, 4, 8, 9, 10, 11], 'leaves task 1 with no path'),
                     ([0, 5], 'leaves task 2 with no path')):
        with pytest.raises(_lib.PrompError, match=msg):
            ctx.set_step_selection(K, bad)
    idx = np.asarray(good, np.int32)
    with pytest.raises(_lib.PrompError, match='negative'):
        ctx._call('promp_set_step_selection', K, -1, idx.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32)))
    with pytest.raises(_lib.PrompError, match='out of range'):
        ctx.set_step_selection(K + 1, good)
    assert ctx.state_version() == ver and ctx.step_selection(K) == len(good)
    assert np.array_equal(ctx.constraint_hvp(v, refresh_chain=True), h)
    fresh = make_ctx(lib, len(lengths), O, A, hidden, K, all_paths)
    with pytest.raises(_lib.PrompError, match='no data'):
        fresh.set_step_selection(0, good)
    fresh.close()
    ctx.close()


# ---- plugin level -----------------------------------------------------------------------------------------------------------

def _trpo_step(lib, theta, all_slabs, M, P, O, A, hidden, K, hv, factor, device_solve=True, seed=1234, by_hand=False):
    """one TRPOMAML.optimize_policy from `theta` with np.random seeded -> optimizer.last (a copy); by_hand: also the direction and
    the step length of the same draw set through the Context, the library's solve and the optimizer's own formula"""
    from promp_amd import session
    from promp_amd.meta_algos.trpo_maml import TRPOMAML
    from promp_amd.policies.meta_gaussian_mlp_policy import MetaGaussianMLPPolicy
    from promp_amd.utils import logger
    logger.configure(quiet=True)
    _lib.set_library_for_testing(lib)
    try:
        spec = op.PolicySpec(O, A, hidden)
        policy = MetaGaussianMLPPolicy(name='p', obs_dim=O, action_dim=A, meta_batch_size=M, hidden_sizes=hidden)
        policy.set_params(spec.to_ordered_dict(theta))
        kw = {} if factor is None else dict(subsample_factor=factor)
        algo = TRPOMAML(policy=policy, step_size=0.01, inner_type='log_likelihood', inner_lr=0.05, meta_batch_size=M,
                        num_inner_grad_steps=K, hvp_approach=hv, **kw)
        algo.optimizer._cg_iters, algo.optimizer._max_backtracks, algo.optimizer._device_solve = 3, 2, device_solve
        samples = [[dict(observations=d['observations'], actions=d['actions'], advantages=d['advantages'], agent_infos=d['agent_infos'],
                         path_lengths=[len(d['advantages']) // P] * P) for d in step] for step in all_slabs]
        np.random.seed(seed)
        algo.optimize_policy(samples, log=False)
        last = dict(algo.optimizer.last)
        ctx = algo.session.ctx
        assert [ctx.step_selection(k) for k in range(K + 1)] == [0] * (K + 1)      # cleared after the closing product
        if by_hand:
            np.random.seed(seed)
            n = last['subsample_paths']
            ctx.set_theta(theta)
            for k in range(K + 1):
                tpo = ctx.step_tpo[k]
                ctx.set_step_selection(k, np.concatenate([tpo[i] + np.sort(np.random.choice(int(tpo[i + 1] - tpo[i]), n[k][i], replace=False))
                                                          for i in range(M)]))
            x, q = ctx.cg_solve(last['gradient'], cg_iters=3, hvp_mode=2 if hv == 'exact' else 0, inner_kind=_lib.INNER_LOGLIK)
            ctx.clear_selections()
            last['by_hand'] = (x, float(np.sqrt(2.0 * 0.01 * (1. / (q + 1e-8)))))
        return last
    finally:
        _lib.set_library_for_testing(None)
        session._current = None


def check_plugin(lib, seed, O=5, A=3, hidden=(32, 32), K=1, T=20, modes=('exact', 'finite_difference')):
    """item 6: TRPOMAML on an on-policy batch of 3 tasks with 4 paths each"""
    from promp_amd.optimizers.conjugate_gradient_optimizer import ConjugateGradientOptimizer, subsample_counts
    M, P = 3, 4
    alpha = np.full(op.PolicySpec(O, A, hidden).n_params, 0.05, np.float32)
    theta, all_slabs, _ = on_policy_case(seed, M, P, T, O, A, hidden, K, alpha, pm.INNER_LOGLIK, ragged=False)
    for bad in (0, -0.1, 1.5):
        with pytest.raises(ValueError):
            ConjugateGradientOptimizer(subsample_factor=bad)
    assert subsample_counts(0.5, [P] * M) == [2] * M
    args = (lib, theta, all_slabs, M, P, O, A, hidden, K)
    for hv in modes:
        # same draw, same step: the selection set by hand, the library's solve, the optimizer's own step length
        half = _trpo_step(*args, hv, 0.5, by_hand=True)
        assert half['subsample_paths'] == [[2, 2, 2]] * (K + 1)
        assert np.array_equal(half['descent_direction'], half['by_hand'][0]) and half['initial_step_size'] == half['by_hand'][1]
        # fails without the feature: half the paths give another direction than all of them
        full = _trpo_step(*args, hv, 1.)
        assert full['subsample_paths'] is None
        assert np.array_equal(full['gradient'], half['gradient'])               # the loss gradient is the whole batch's either way
        assert not np.array_equal(full['descent_direction'], half['descent_direction'])
        # defaults: 1. is what leaving it unset gives
        unset = _trpo_step(*args, hv, None)
        assert np.array_equal(unset['descent_direction'], full['descent_direction'])
        assert unset['initial_step_size'] == full['initial_step_size']
        if hv == 'exact':
            # the host loop over the same products: to check_cg_solve_on_device's tolerance for the exact mode
            host = _trpo_step(*args, hv, 0.5, device_solve=False)
            assert host['subsample_paths'] == [[2, 2, 2]] * (K + 1)
            assert rel_max(host['descent_direction'], half['descent_direction'].astype(np.float64)) < 2e-4
