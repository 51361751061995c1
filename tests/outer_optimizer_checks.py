"""The outer optimiser's rule, its arguments and the clip by the global norm (promp_set_outer_optimizer), shared by
test_emu_outer_optimizer.py (emulator, tiny) and test_gpu_outer_optimizer.py (-m gpu).

Float64 mirrors of the three rules (TF1 semantics, include/promp_hip.h) and of the clip, and where every bound comes from:

(1) The rule alone (check_rule).  The device's own inputs -- float32(red * inv_tasks), the slots and parameters read back before
    the step -- go through the mirror in float64.  A rule is at most eight float32 operations per output, each correctly rounded
    (2^-24 = 6e-8 relative); the error an output inherits from its operands is relative to THEIR magnitude, so every output is
    held to 1e-6 x (the largest operand magnitude of the output's last operation) -- for m = b1 m + (1 - b1) g that is
    max(|b1 m|, |(1 - b1) g|), for theta = theta - u it is max(|theta|, |u|) -- plus 2^-24 |theta| for theta, whose own rounding is
    relative to theta and not to the update.  Whether the compiler contracts a multiply-add changes one rounding and nothing in
    this bound.  The norm's square is accumulated in float64 (2^-53 per addition: nothing) and rounded to float32 once after the
    root: 2^-24 = 6e-8, held to 2e-7 relative of the float64 norm of the same float32 entries.  The mirror takes the float32 norm
    the device reports into the scale, as the kernel does.

(2), (3), (5) need no tolerance: two device paths that must do the same float32 operations in the same order.

(4) End to end against the float64 oracle (oracle.promp.meta_objective_and_grad; step_size_checks.analytic for the joint norm).
    Adam with other arguments: parity_checks.assert_adam_trajectory as it stands, pm.adam_step(b1, b2, eps) as the reference.
    SGD, Momentum and the clip are LINEAR in the gradients: with |g_dev - g_ref| <= 1e-4 max|g| per epoch (the project's functional
    tolerance of a device meta-gradient, parity_checks), theta after E epochs differs by at most lr x 1e-4 x max|g| x gain, where
    the gain is how much of a unit gradient error per epoch reaches theta: E for SGD; sum_{e=1..E} (1 - mu^e) / (1 - mu) for
    Momentum (the accumulator after e epochs holds sum_{i<e} mu^i of it).  An ACTIVE clip multiplies g by c / n <= 1: the error of
    g enters scaled by at most 1, and the norm's own relative error (<= 1e-4, it is a norm of the same gradient) enters once more
    times |g| c / n <= max|g|: twice the bound.  max|g| is the largest over the epochs
    of the oracle's max-norm.  The learning rate of these runs is 0.5: the bound then sits two orders above theta's float32
    spacing (2^-24 |theta| ~ 6e-8 per step against 0.5 x 1e-4 x max|g| ~ 1e-6 .. 1e-5), which a learning rate of 1e-3 would not.
"""
import os

import numpy as np
import pytest

from oracle import policy as op, promp as pm
from promp_amd import _lib
from tests import minibatch_checks as mb, step_size_checks as sc
from tests.parity_checks import assert_adam_trajectory

CLIP = sc.CLIP
U = 2.0 ** -24

ADAM_ARGS = dict(beta1=0.8, beta2=0.99, epsilon=1e-5)
RULES = {
    'adam': ('adam', ADAM_ARGS),
    'sgd': ('sgd', {}),
    'momentum': ('momentum', dict(momentum=0.9)),
    'nesterov': ('momentum', dict(momentum=0.9, use_nesterov=True)),
}


# ---- float64 mirrors -----------------------------------------------------------------------------------------------------

def f32(x):
    return np.float64(np.float32(x))


def mirror_lr_t(rule, args, lr, t):
    """outer_lr_t (promp_plan.h): Adam's bias-corrected rate in double from the float32 betas, rounded once; lr otherwise"""
    if rule != 'adam':
        return f32(lr)
    b1, b2 = f32(args['beta1']), f32(args['beta2'])
    return f32(f32(lr) * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t))


def mirror_clip(g_parts, c):
    """-> (float64 norm over all parts, scale): n > c ? c / n : 1 with n rounded to float32 first; non-finite n: NaN"""
    n64 = float(np.sqrt(sum(np.sum(np.asarray(g, np.float64) ** 2) for g in g_parts)))
    if not c:
        return n64, 1.0
    n = f32(n64)
    if not np.isfinite(n):
        return n64, float('nan')
    return n64, (f32(c) / n if n > f32(c) else 1.0)


def mirror_rule(rule, args, p, s1, s2, g, lr_t, s1_dev, s2_dev):
    """One step of every entry in float64 -> (p', s1', s2', bounds (p, s1, s2)).  The slots from the slots before the step; the
    parameter from the slots the DEVICE wrote (s1_dev, s2_dev: float32 values, each held to its own bound here), so that the
    parameter's bound need not carry what a cancellation in b1 m + (1 - b1) g leaves relative to m.  The bounds are 1e-6 x the
    largest operand of each output's last operation (+ 2^-24 |p| for the parameter), see the module docstring."""
    p, s1, s2, g, s1_dev, s2_dev = (np.asarray(x, np.float64) for x in (p, s1, s2, g, s1_dev, s2_dev))
    zero = np.zeros_like(p)
    if rule == 'adam':
        b1, b2, eps = f32(args['beta1']), f32(args['beta2']), f32(args['epsilon'])
        omb1, omb2 = f32(1.0 - b1), f32(1.0 - b2)
        m, v = b1 * s1 + omb1 * g, b2 * s2 + omb2 * g * g
        u = lr_t * s1_dev / (np.sqrt(s2_dev) + eps)
        bm = 1e-6 * np.maximum(np.abs(b1 * s1), np.abs(omb1 * g))
        bv = 1e-6 * np.maximum(np.abs(b2 * s2), np.abs(omb2 * g * g))
        return p - u, m, v, (1e-6 * np.maximum(np.abs(p), np.abs(u)) + U * np.abs(p), bm, bv)
    if rule == 'sgd':
        u = lr_t * g
        return p - u, s1, s2, (1e-6 * np.maximum(np.abs(p), np.abs(u)) + U * np.abs(p), zero, zero)
    mu = f32(args['momentum'])
    a = mu * s1 + g
    u = lr_t * (g + mu * s1_dev if args.get('use_nesterov') else s1_dev)
    ba = 1e-6 * np.maximum(np.abs(mu * s1), np.abs(g))
    return p - u, a, s2, (1e-6 * np.maximum(np.abs(p), np.abs(u)) + U * np.abs(p), ba, zero)


def momentum_gain(mu, E):
    return sum((1.0 - mu ** e) / (1.0 - mu) for e in range(1, E + 1))


# ---- helpers ---------------------------------------------------------------------------------------------------------------

def state(ctx, sizes=False):
    m, v, t = ctx.get_adam_state()
    s = dict(theta=ctx.get_theta(), m=m, v=v, t=t)
    if sizes:
        s['alpha'] = ctx.get_step_sizes()
        s['am'], s['av'] = ctx.get_step_size_adam_state()
    return s


def same_state(a, b):
    assert a['t'] == b['t'], (a['t'], b['t'])
    assert sorted(a) == sorted(b)
    for k in a:
        if k != 't':
            assert np.array_equal(a[k], b[k]), (k, float(np.max(np.abs(a[k].astype(np.float64) - b[k]))))


def oracle_grads(case, sizes=False):
    """the float64 oracle's task-mean gradient at the case's parameters (with sizes: theta's and alpha's) and their joint norm"""
    if sizes:
        r = sc.analytic(case.spec, case.t64, case.all_slabs, case.a64, case.e64)
        parts = [r['grad'], r['grad_alpha']]
    else:
        parts = [pm.meta_objective_and_grad(case.spec, case.t64, case.all_slabs, case.a64, case.e64, CLIP)['grad']]
    return parts, float(np.sqrt(sum(np.sum(g ** 2) for g in parts)))


# ---- (1) the rule alone ------------------------------------------------------------------------------------------------------

def check_rule(lib, case, key, clip, learn_std=True, sizes=False, steps=3, lr=1e-2):
    """meta_grad -> reduced_get -> adam_step, `steps` times (the slots are non-zero from the second on): every output of every step
    against the mirror on the device's own inputs.  clip: the first step's norm is halved, the later ones as they fall."""
    rule, args = RULES[key]
    n, K, A, M = case.n, case.K, case.A, case.M
    ctx = case.ctx(lib)
    if not learn_std:
        ctx.set_learn_std(False)
    if sizes:
        ctx.set_train_step_sizes(True)
    nt = n if learn_std else n - A
    inv = np.float32(1.0) / np.float32(M)
    worst = 0.0
    c = None
    for step in range(1, steps + 1):
        ctx.meta_grad(CLIP, case.eta)
        red = ctx.reduced_get()
        g = (red[:n] * inv).astype(np.float32)
        ga = (red[n + K + 2:] * inv).astype(np.float32) if sizes else None
        parts = [g[:nt]] + ([ga[:nt]] if sizes else [])
        if clip and c is None:
            c = float(np.float32(0.5 * mirror_clip(parts, 0)[0]))
        if step == 1:
            ctx.set_outer_optimizer(rule, args, max_grad_norm=c)
            if not clip:
                with pytest.raises(_lib.PrompError, match='clipping is off'):
                    ctx.grad_norm()
        before = state(ctx, sizes)
        assert before['t'] == step - 1
        ctx.adam_step(lr)
        after = state(ctx, sizes)
        assert after['t'] == step
        n64, scale = mirror_clip(parts, c)
        if clip:
            got = ctx.grad_norm()
            assert abs(got - n64) <= 2e-7 * n64, (got, n64)
            scale = f32(c) / f32(got) if f32(got) > f32(c) else 1.0        # (the device's own float32 norm enters the scale)
            if step == 1:
                assert scale < 1.0
        lr_t = mirror_lr_t(rule, args, lr, step)

        def judge(p0, s10, s20, gg, p1, s11, s21, what):
            w = 0.0
            ep, e1, e2, (bp, b1_, b2_) = mirror_rule(rule, args, p0[:nt], s10[:nt], s20[:nt], gg[:nt].astype(np.float64) * scale, lr_t,
                                                     s11[:nt], s21[:nt])
            for got_, exp, bound, name in ((p1, ep, bp, 'p'), (s11, e1, b1_, 's1'), (s21, e2, b2_, 's2')):
                err = np.abs(got_[:nt].astype(np.float64) - exp)
                assert np.all(err <= bound), (what, name, step, float(np.max(err - bound)))
                w = max(w, float(np.max(err / np.where(bound > 0, bound, 1.0))))
            # entries that are not trained: neither stepped nor slotted
            for x0, x1 in ((p0, p1), (s10, s11), (s20, s21)):
                assert np.array_equal(x0[nt:], x1[nt:]), what
            return w
        worst = max(worst, judge(before['theta'], before['m'], before['v'], g, after['theta'], after['m'], after['v'], 'theta'))
        if sizes:
            worst = max(worst, judge(before['alpha'], before['am'], before['av'], ga, after['alpha'], after['am'], after['av'], 'alpha'))
        assert not np.array_equal(after['theta'][:nt], before['theta'][:nt])
    ctx.close()
    print('%s clip=%s learn_std=%s sizes=%s: worst error %.3f of its bound' % (key, clip, learn_std, sizes, worst))


# ---- (2) the forced general instance ----------------------------------------------------------------------------------------------

def check_generic_equals_plain(lib, case, monkeypatch, epochs=2):
    """PROMP_OUTER_GENERIC=1 (read when a context is created) against unset, default arguments: fused and split, with and without
    trained step sizes, bit for bit"""
    def run(generic, split, sizes):
        if generic:
            monkeypatch.setenv('PROMP_OUTER_GENERIC', '1')
        else:
            monkeypatch.delenv('PROMP_OUTER_GENERIC', raising=False)
        ctx = case.ctx(lib)
        monkeypatch.delenv('PROMP_OUTER_GENERIC', raising=False)
        if sizes:
            ctx.set_train_step_sizes(True)
        if split:
            ctx.comm_split_path(True)
        r = ctx.optimize(epochs, 1e-3, CLIP, case.eta)
        out = (state(ctx, sizes), r)
        ctx.close()
        return out
    for split in (False, True):
        for sizes in (False, True):
            (s0, r0), (s1, r1) = run(False, split, sizes), run(True, split, sizes)
            same_state(s0, s1)
            assert r0['loss_before'] == r1['loss_before'] and r0['loss_after'] == r1['loss_after']
            assert s0['t'] == epochs and not np.array_equal(s0['theta'], case.theta)


# ---- (3) an inactive clip ------------------------------------------------------------------------------------------------------

def check_inactive_clip(lib, case, epochs=3, sizes=False):
    """max_grad_norm = 10 x the oracle's first-epoch norm: scale == 1 exactly, and the split route the clip takes is the fused one"""
    _, n0 = oracle_grads(case, sizes)
    out = []
    for c in (None, 10.0 * n0):
        ctx = case.ctx(lib)
        if sizes:
            ctx.set_train_step_sizes(True)
        if c:
            ctx.set_outer_optimizer('adam', None, max_grad_norm=c)
        ctx.optimize(epochs, 1e-3, CLIP, case.eta)
        if c:
            assert 0.0 < ctx.grad_norm() < c
        out.append(state(ctx, sizes))
        ctx.close()
    same_state(out[0], out[1])


# ---- (4) end to end against the float64 oracle -----------------------------------------------------------------------------------

def adam_oracle_trajectory(case, epochs, lr):
    b1, b2, eps = f32(ADAM_ARGS['beta1']), f32(ADAM_ARGS['beta2']), f32(ADAM_ARGS['epsilon'])
    th, st, gmin, gmax = case.t64.copy(), pm.AdamState(case.n), None, []
    for _ in range(epochs):
        g = pm.meta_objective_and_grad(case.spec, th, case.all_slabs, case.a64, case.e64, CLIP)['grad']
        gmin = np.abs(g) if gmin is None else np.minimum(gmin, np.abs(g))
        gmax.append(np.max(np.abs(g)))
        th = pm.adam_step(th, g, st, lr, b1=b1, b2=b2, eps=eps)
    return th, st, gmin, np.array(gmax)


def check_adam_arguments(lib, case, epochs=3, lr=1e-3):
    th, st, gmin, gmax = adam_oracle_trajectory(case, epochs, lr)
    ctx = case.ctx(lib)
    ctx.set_outer_optimizer('adam', ADAM_ARGS)
    ctx.optimize(epochs, lr, CLIP, case.eta)
    m, v, t = ctx.get_adam_state()
    assert t == epochs
    worst = assert_adam_trajectory(ctx.get_theta().astype(np.float64) - case.t64, th - case.t64, gmin, gmax, lr, epochs,
                                   m_dev=m, v_dev=v, m_ref=st.m, v_ref=st.v)
    print('Adam(0.8, 0.99, 1e-5): worst judged entry %.3e of one step, %.1f %% below the floor' % (worst[0], 100 * worst[1]))
    # and it is not what the default arguments give
    ctx2 = case.ctx(lib)
    ctx2.optimize(epochs, lr, CLIP, case.eta)
    assert not np.array_equal(ctx2.get_theta(), ctx.get_theta())
    ctx.close()
    ctx2.close()


LINEAR_LR = 0.5


def check_linear_rule(lib, case, key, clip, epochs=3, lr=LINEAR_LR):
    """SGD / Momentum, clip off or active (c = half the oracle's first-epoch norm), E epochs of optimize() against the
    float64 loop; bound: module docstring (4)"""
    rule, args = RULES[key]
    assert rule != 'adam' and not args.get('use_nesterov')
    _, n0 = oracle_grads(case)
    c = 0.5 * n0 if clip else None
    th, a, gmax = case.t64.copy(), np.zeros(case.n), 0.0
    mu = f32(args.get('momentum', 0.0))
    for e in range(epochs):
        g = pm.meta_objective_and_grad(case.spec, th, case.all_slabs, case.a64, case.e64, CLIP)['grad']
        gmax = max(gmax, float(np.max(np.abs(g))))
        if c:
            n = float(np.sqrt(np.sum(g ** 2)))
            if e == 0:
                assert n > c
            g = g * (c / n if n > c else 1.0)
        if rule == 'sgd':
            th = th - lr * g
        else:
            a = mu * a + g
            th = th - lr * a
    gain = float(epochs) if rule == 'sgd' else momentum_gain(mu, epochs)
    bound = lr * 1e-4 * gmax * gain * (2.0 if c else 1.0)
    ctx = case.ctx(lib)
    ctx.set_outer_optimizer(rule, args, max_grad_norm=c)
    ctx.optimize(epochs, lr, CLIP, case.eta)
    _, _, t = ctx.get_adam_state()
    assert t == epochs
    err = np.max(np.abs((ctx.get_theta().astype(np.float64) - case.t64) - (th - case.t64)))
    print('%s clip=%s: max |d theta_dev - d theta_ref| %.3e, bound %.3e (max|g| %.3e, gain %.3f)' % (key, bool(c), err, bound, gmax, gain))
    ctx.close()
    assert np.max(np.abs(th - case.t64)) > 100 * bound          # the trajectory is far longer than what it is held to
    assert err <= bound, (err, bound)


# ---- (5) routes ---------------------------------------------------------------------------------------------------------------

def check_routes_with_clip(lib, case, key='adam', epochs=2, sizes=False, lr=1e-3, comm=True):
    """clipping on (active: half the oracle's first-epoch norm): optimize(E) against the caller's own exchange
    (meta_grad -> reduced_get -> reduced_set -> adam_step), and (comm; a rendezvous costs over a second) against a one-rank
    communicator with and without the fixed-order exchange -- bit for bit, the norm included"""
    rule, args = RULES[key]
    _, n0 = oracle_grads(case, sizes)
    c = 0.5 * n0

    def make(comm=False, fixed=False):
        ctx = case.ctx(lib)
        if sizes:
            ctx.set_train_step_sizes(True)
        ctx.set_outer_optimizer(rule, args, max_grad_norm=c)
        if comm:
            ctx.comm_init(0, 1, _lib.comm_unique_id(lib))
            ctx.comm_fixed_order(fixed)
        return ctx
    ctx = make()
    ctx.optimize(epochs, lr, CLIP, case.eta)
    ref, ref_norm = state(ctx, sizes), ctx.grad_norm()
    assert ref_norm > c or epochs > 1
    ctx.close()
    ctx = make()
    for _ in range(epochs):
        ctx.meta_grad(CLIP, case.eta)
        ctx.reduced_set(ctx.reduced_get().copy())
        ctx.adam_step(lr)
    same_state(ref, state(ctx, sizes))
    assert ctx.grad_norm() == ref_norm
    ctx.close()
    for fixed in ((False, True) if comm else ()):
        ctx = make(comm=True, fixed=fixed)
        ctx.optimize(epochs, lr, CLIP, case.eta)
        same_state(ref, state(ctx, sizes))
        assert ctx.grad_norm() == ref_norm
        ctx.close()


# ---- (8) the final stage's grid edges ------------------------------------------------------------------------------------------

# Single-hidden-layer shapes (the layer-by-layer kernels; the final stage does not depend on the pass family) whose
# Theta = H (O + 1 + A) + 2 A puts the scalar columns, the statistics thread and the last block on the edges of the final stage's
# grids (final_stage_launch, promp_plan.h): 64 columns per reduce block, 256 threads per mean block.
EDGE_SHAPES = {
    # Theta 62: the scalar columns 62 .. 65 straddle two blocks; with trained step sizes 2 Theta + K + 2 = 128, an exactly full grid
    'theta62': dict(M=2, O=4, A=4, hidden=(6,), K=2),
    # Theta 60: Theta + K + 2 = 64, exactly one full reduce block
    'theta60': dict(M=2, O=5, A=3, hidden=(6,), K=2),
    # Theta 255: the surrogate's sum is a block's last column; the mean kernel's statistics thread is a block's last
    'theta255': dict(M=2, O=8, A=4, hidden=(19,), K=1),
    # Theta 256: the surrogate's sum opens a block, the statistics thread opens the second mean block, 2 Theta + 1 = 513 leaves one
    # thread in the last; five tasks over four task quarters
    'theta256': dict(M=5, O=6, A=3, hidden=(25,), K=1),
}
_edge_cases = {}


def edge_case(name):
    if name not in _edge_cases:
        _edge_cases[name] = sc.PrompCase(720 + sorted(EDGE_SHAPES).index(name), P=1, T=20, ragged=True, **EDGE_SHAPES[name])
        assert _edge_cases[name].n == int(name[5:])
    return _edge_cases[name]


def oracle_task_scalars(case):
    """the float64 oracle's per-task scalars [M][K + 2]: J_i, KL^k_i, outer KL_i (computed once per case)"""
    if getattr(case, '_task_scalars', None) is None:
        rows = []
        for i in range(case.M):
            r = pm.meta_objective_and_grad(case.spec, case.t64, case.all_slabs, case.a64, case.e64, CLIP, want_grad=False,
                                           tasks=[i], n_tasks_total=1)
            rows.append(np.concatenate([[r['loss'] - np.mean(case.e64 * r['inner_kl'])], r['inner_kl'], [r['outer_kl']]]))
        case._task_scalars = np.array(rows)
    return case._task_scalars


def check_stats_against_exchange(lib, case):
    """The statistics row against the exchange buffer it is computed from, after meta_grad on the fused and on the forced split
    route, step sizes fixed and trained.  The KL entries are ONE float32 multiplication each: exact.  The loss is
    red[Theta] inv + (sum_k eta_k KL_k) / K: a product, the penalty's sum and quotient and the closing addition -- three roundings
    of values no larger than the two terms, and a contraction of eta_k KL_k into the sum changes one of them -- held to
    4 x 2^-24 of the terms' magnitudes.  The scalar sums themselves against the float64 oracle's per-task values at parity_checks'
    tolerance for a loss or a KL (rtol 1e-4, atol 1e-6), summed over the tasks as the column is.  The routes: bit for bit."""
    n, K, M = case.n, case.K, case.M
    inv = np.float32(1.0) / np.float32(M)
    eta = case.eta.astype(np.float32)
    want = oracle_task_scalars(case)
    bound = np.sum(1e-6 + 1e-4 * np.abs(want), axis=0)

    def run(split, sizes):
        ctx = case.ctx(lib)
        if sizes:
            ctx.set_train_step_sizes(True)
        if split:
            ctx.comm_split_path(True)
        g, st = ctx.meta_grad(CLIP, case.eta)
        out = dict(g=g, red=ctx.reduced_get(), stats=np.concatenate([[st['loss']], st['inner_kl'], [st['outer_kl']]]).astype(np.float32))
        if sizes:
            out['ga'] = ctx.get_step_size_grad()
        ctx.close()
        return out
    for sizes in (False, True):
        fused, split = run(False, sizes), run(True, sizes)
        assert sorted(fused) == sorted(split)
        for key in fused:
            assert np.array_equal(fused[key], split[key]), (sizes, key)
        red, stats = fused['red'], fused['stats']
        assert red.shape == ((2 if sizes else 1) * n + K + 2,) and red.dtype == np.float32
        for k in range(K + 1):
            assert stats[1 + k] == np.float32(red[n + 1 + k] * inv), (sizes, k, stats[1 + k], red[n + 1 + k])
        j64 = np.float64(red[n]) * np.float64(inv)
        pen = [np.float64(eta[k]) * np.float64(stats[1 + k]) / K for k in range(K)]
        err, lim = abs(np.float64(stats[0]) - (j64 + sum(pen))), 4.0 * U * (abs(j64) + sum(abs(p) for p in pen))
        print('sizes=%s: |loss - float64| %.3e, bound %.3e' % (sizes, err, lim))
        assert err <= lim, (sizes, err, lim)
        err = np.abs(red[n:n + K + 2].astype(np.float64) - np.sum(want, axis=0))
        print('sizes=%s: scalar sums against the oracle, worst %.3f of the bound' % (sizes, float(np.max(err / bound))))
        assert np.all(err <= bound), (sizes, err, bound)
        assert np.array_equal(fused['g'], (red[:n] * inv).astype(np.float32))


def check_minibatch_sgd_clip(lib, seed, O=5, A=3, hidden=(32, 32), K=1, lengths=mb.LENGTHS, pattern=mb.ASSIGN_2, max_grad_norm=1e-3):
    """optimize_minibatch(B = 2) under SGD with the clip on against the same steps one by one on truncated batches:
    minibatch_checks' own construction, every context of it given the settings"""
    class Case(mb.Case):
        def fresh(self, paths, slabs):
            ctx = mb.Case.fresh(self, paths, slabs)
            ctx.set_outer_optimizer('sgd', None, max_grad_norm=max_grad_norm)
            return ctx
    c = Case(lib, seed, O, A, hidden, K, lengths=lengths)
    assign = [mb.per_step(pattern, 2, K)]
    c.ctx.optimize_minibatch(1, 2, assign, mb.LR, mb.CLIP, mb.eta_of(K))
    got, norm = c.get(c.ctx), c.ctx.grad_norm()
    want = c.by_hand(assign, 2, c.zero_state(), _lib.INNER_RATIO)
    mb.same_state(got, want)
    assert got['t'] == 2 and not np.array_equal(got['theta'], c.theta)
    assert np.all(got['m'] == 0.0) and np.all(got['v'] == 0.0)          # SGD keeps no slots
    assert norm > max_grad_norm                                        # the clip was active in the last step
    c.close()


# ---- (6) state -------------------------------------------------------------------------------------------------------------------

def check_state(lib, case):
    ctx = case.ctx(lib)
    ctx.set_train_step_sizes(True)
    assert ctx.get_outer_optimizer() == dict(rule='adam', args=dict(beta1=float(np.float32(0.9)), beta2=float(np.float32(0.999)),
                                                                    epsilon=float(np.float32(1e-8))), max_grad_norm=None)
    ctx.optimize(2, 1e-3, CLIP, case.eta)
    s = state(ctx, True)
    assert s['t'] == 2 and np.any(s['m'] != 0) and np.any(s['am'] != 0)
    ctx.set_outer_optimizer('adam', dict(epsilon=1e-5), max_grad_norm=0.25)      # new arguments: everything stays
    same_state(s, state(ctx, True))
    got = ctx.get_outer_optimizer()
    assert got['rule'] == 'adam' and got['max_grad_norm'] == 0.25 and got['args']['epsilon'] == float(np.float32(1e-5))
    ctx.set_outer_optimizer('momentum', dict(momentum=0.9))                      # a new rule: slots and step count start over
    z = state(ctx, True)
    assert z['t'] == 0 and not any(np.any(z[k] != 0) for k in ('m', 'v', 'am', 'av'))
    assert np.array_equal(z['theta'], s['theta']) and np.array_equal(z['alpha'], s['alpha'])
    assert ctx.get_outer_optimizer() == dict(rule='momentum', args=dict(momentum=float(np.float32(0.9)), use_nesterov=False), max_grad_norm=None)
    # set / get round trip under Momentum; the slot the rule does not use is carried along
    rng = np.random.RandomState(case.seed + 9)
    m, v = rng.randn(case.n).astype(np.float32), rng.rand(case.n).astype(np.float32)
    ctx.set_adam_state(m, v, 7)
    m2, v2, t2 = ctx.get_adam_state()
    assert np.array_equal(m, m2) and np.array_equal(v, v2) and t2 == 7
    ctx.meta_grad(CLIP, case.eta)
    ctx.adam_step(1e-2)
    m3, v3, t3 = ctx.get_adam_state()
    assert t3 == 8 and np.array_equal(v3, v) and not np.array_equal(m3, m)
    ctx.close()


def check_session_keeps_settings(lib):
    """a context regrown by session.ensure carries the rule, its arguments and the clip"""
    from promp_amd import session
    _lib.set_library_for_testing(lib)
    try:
        s = session.DeviceSession(2, 5, 3, (32, 32), 1)
        s.set_theta(np.zeros(op.PolicySpec(5, 3, (32, 32)).n_params, np.float32))
        s.set_outer_optimizer(type('MomentumOptimizer', (), {}), dict(momentum=0.5, use_nesterov=True), max_grad_norm=2.0)
        ctx = s.ensure(100, 4)
        want = dict(rule='momentum', args=dict(momentum=0.5, use_nesterov=True), max_grad_norm=2.0)
        assert ctx.get_outer_optimizer() == want
        ctx2 = s.ensure(1000, 40)
        assert ctx2 is not ctx and ctx2.get_outer_optimizer() == want
        g = s.get_outer_optimizer()
        assert g['rule'] == 'momentum' and g['max_grad_norm'] == 2.0 and np.array_equal(g['args'], np.array([0.5, 1, 0, 0], np.float32))
        with pytest.raises(_lib.PrompError, match='RMSPropOptimizer'):
            s.set_outer_optimizer(type('RMSPropOptimizer', (), {}))
        assert ctx2.get_outer_optimizer() == want
        s.ctx.close()
    finally:
        _lib.set_library_for_testing(None)
        session._current = None


# ---- (7) refusals ------------------------------------------------------------------------------------------------------------------

def check_refusals(lib, case):
    from promp_amd.optimizers.maml_first_order_optimizer import MAMLFirstOrderOptimizer
    ctx = case.ctx(lib)
    ctx.set_outer_optimizer('momentum', dict(momentum=0.5), max_grad_norm=None)
    ctx.meta_grad(CLIP, case.eta)
    ctx.adam_step(1e-2)
    before, settings = state(ctx), ctx.get_outer_optimizer()

    def refused(msg, call):
        with pytest.raises(_lib.PrompError, match=msg):
            call()
        same_state(state(ctx), before)
        assert ctx.get_outer_optimizer() == settings
    refused('RMSPropOptimizer', lambda: ctx.set_outer_optimizer(type('RMSPropOptimizer', (), {})))
    refused("'rmsprop'", lambda: ctx.set_outer_optimizer('rmsprop'))
    refused('rule 7 unknown', lambda: ctx.set_outer_optimizer(7))
    refused("'beta3'", lambda: ctx.set_outer_optimizer('adam', dict(beta3=0.5)))
    refused("'momentum'.*adam", lambda: ctx.set_outer_optimizer('adam', dict(momentum=0.5)))
    refused('beta1', lambda: ctx.set_outer_optimizer('adam', dict(beta1=1.0)))
    refused('epsilon', lambda: ctx.set_outer_optimizer('adam', dict(epsilon=0.0)))
    # (the library's own checks, behind the binding's: the float[4] goes straight through)
    refused('beta1 1 outside', lambda: ctx.set_outer_optimizer(0, np.array([1.0, 0.999, 1e-8, 0], np.float32)))
    refused('beta2 .* outside', lambda: ctx.set_outer_optimizer(0, np.array([0.9, -0.1, 1e-8, 0], np.float32)))
    refused('epsilon 0 must be positive', lambda: ctx.set_outer_optimizer(0, np.array([0.9, 0.999, 0.0, 0], np.float32)))
    refused('momentum 1 outside', lambda: ctx.set_outer_optimizer(2, np.array([1.0, 0, 0, 0], np.float32)))
    refused('max_grad_norm', lambda: ctx.set_outer_optimizer('sgd', None, max_grad_norm=-1.0))
    refused('max_grad_norm', lambda: ctx.set_outer_optimizer('sgd', None, max_grad_norm=float('inf')))
    refused('max_grad_norm', lambda: ctx.set_outer_optimizer('sgd', None, max_grad_norm=float('nan')))
    refused('clipping is off', lambda: ctx.grad_norm())
    ctx.close()
    # the optimiser object refuses what it used to accept and ignore
    with pytest.raises(_lib.PrompError, match='RMSPropOptimizer'):
        MAMLFirstOrderOptimizer(tf_optimizer_cls=type('RMSPropOptimizer', (), {}))
    with pytest.raises(_lib.PrompError, match="'decay'"):
        MAMLFirstOrderOptimizer(tf_optimizer_args=dict(decay=0.9))
    o = MAMLFirstOrderOptimizer(tf_optimizer_cls=type('GradientDescentOptimizer', (), {}), tf_optimizer_args=dict(learning_rate=0.3))
    assert o._rule == _lib.OUTER_RULES['sgd'] and o._learning_rate == 0.3
    assert _lib.outer_rule_id(None) == _lib.outer_rule_id('adam') == _lib.outer_rule_id(type('AdamOptimizer', (), {})) == 0
    assert _lib.outer_rule_id('gradient_descent') == _lib.outer_rule_id('sgd') == 1 and _lib.outer_rule_id('momentum') == 2


# ---- (9) plugins -------------------------------------------------------------------------------------------------------------------

def build_trainer(algo_name, n_itr, log_dir=None, **algo_kw):
    """step_size_checks.build_trainer's point-environment trainer with the outer optimiser's arguments passed on"""
    from promp_amd.baselines.linear_baseline import LinearFeatureBaseline, LinearTimeBaseline
    from promp_amd.envs.normalized_env import normalize
    from promp_amd.envs.point_env import MetaPointEnvCorner
    from promp_amd.meta_algos.dice_maml import DICEMAML
    from promp_amd.meta_algos.pro_mp import ProMP
    from promp_amd.meta_algos.vpg_maml import VPGMAML
    from promp_amd.meta_trainer import Trainer
    from promp_amd.policies.meta_gaussian_mlp_policy import MetaGaussianMLPPolicy
    from promp_amd.samplers.device_point_sampler import DevicePointEnvSampler
    from promp_amd.samplers.dice_sample_processor import DiceMetaSampleProcessor
    from promp_amd.samplers.meta_sample_processor import MetaSampleProcessor
    from promp_amd.utils import logger
    logger.configure(dir=log_dir, snapshot_mode='last', quiet=True)
    np.random.seed(1)
    M, P, T = 2, 3, 12
    env = normalize(MetaPointEnvCorner(reward_type='dense'))
    policy = MetaGaussianMLPPolicy(name='meta-policy', obs_dim=2, action_dim=2, meta_batch_size=M, hidden_sizes=(32, 32))
    sampler = DevicePointEnvSampler(env=env, policy=policy, rollouts_per_meta_task=P, meta_batch_size=M, max_path_length=T, parallel=False)
    common = dict(policy=policy, inner_lr=0.1, meta_batch_size=M, num_inner_grad_steps=1, learning_rate=1e-3, **algo_kw)
    if algo_name == 'dice':
        proc = DiceMetaSampleProcessor(baseline=LinearTimeBaseline(), max_path_length=T, discount=0.99, normalize_adv=True)
        algo = DICEMAML(T, **common)
    else:
        proc = MetaSampleProcessor(baseline=LinearFeatureBaseline(), discount=0.99, gae_lambda=1, normalize_adv=True)
        algo = (VPGMAML(**common) if algo_name == 'vpg' else
                ProMP(num_ppo_steps=2, clip_eps=0.3, init_inner_kl_penalty=5e-4, adaptive_inner_kl_penalty=False, **common))
    return Trainer(algo=algo, policy=policy, env=env, sampler=sampler, sample_processor=proc, n_itr=n_itr, num_inner_grad_steps=1)


def _flat(policy):
    return np.concatenate([np.asarray(v, np.float32).reshape(-1) for v in policy.get_param_values().values()])


def check_promp_plugin(tmp_dir):
    """ProMP(tf_optimizer_args=dict(epsilon=1e-5), max_grad_norm=0.5) on the point environment: GradNorm logged and finite, theta
    moved, algo.optimizer.loss() behind the step is LossAfter; the snapshot carries the settings; one from before them loads as
    Adam's defaults"""
    from promp_amd.utils import logger
    trainer = build_trainer('promp', 2, log_dir=tmp_dir, tf_optimizer_args=dict(epsilon=1e-5), max_grad_norm=0.5)
    th0 = _flat(trainer.policy)
    seen = sc.train_and_grab(trainer)
    assert 'GradNorm' in seen and np.isfinite(seen['GradNorm']) and seen['GradNorm'] > 0.0
    assert not np.array_equal(_flat(trainer.policy), th0)
    assert trainer.algo.optimizer.loss() == seen['LossAfter'] == trainer.algo.last_stats['loss_after']
    want = dict(rule='adam', args=dict(beta1=float(np.float32(0.9)), beta2=float(np.float32(0.999)), epsilon=float(np.float32(1e-5))),
                max_grad_norm=0.5)
    assert trainer.policy.session.ctx.get_outer_optimizer() == want
    snap = logger.load_params(os.path.join(tmp_dir, 'params.pkl'))
    oo = snap['outer_optimizer']
    assert oo['rule'] == 'adam' and oo['max_grad_norm'] == 0.5 and np.array_equal(oo['args'], np.array([0.9, 0.999, 1e-5, 0], np.float32))
    m, v, t = trainer.policy.session.ctx.get_adam_state()
    again = build_trainer('promp', 3)                       # built with the defaults: the snapshot brings the settings
    again.load_snapshot(snap)
    ctx = again.policy.session.ensure()
    assert ctx.get_outer_optimizer() == want and again.algo.max_grad_norm == 0.5
    m2, v2, t2 = ctx.get_adam_state()
    assert t2 == t == 4 and np.array_equal(m, m2) and np.array_equal(v, v2)
    old = {k: val for k, val in snap.items() if k != 'outer_optimizer'}
    plain = build_trainer('promp', 3, tf_optimizer_cls='sgd', max_grad_norm=0.5)
    plain.load_snapshot(old)
    got = plain.policy.session.ensure().get_outer_optimizer()
    assert got['rule'] == 'adam' and got['max_grad_norm'] is None and got['args']['epsilon'] == float(np.float32(1e-8))
    # no GradNorm without the argument
    off = build_trainer('promp', 1)
    assert 'GradNorm' not in sc.train_and_grab(off)


def check_other_plugin(algo_name):
    """one iteration under 'sgd': theta moves, no slot does, the step count advances"""
    trainer = build_trainer(algo_name, 1, tf_optimizer_cls='sgd')
    th0 = _flat(trainer.policy)
    seen = sc.train_and_grab(trainer)
    assert 'GradNorm' not in seen and np.isfinite(seen['LossAfter'])
    ctx = trainer.policy.session.ctx
    assert ctx.get_outer_optimizer()['rule'] == 'sgd'
    m, v, t = ctx.get_adam_state()
    assert t == 1 and np.all(m == 0.0) and np.all(v == 0.0)
    th1 = _flat(trainer.policy)
    assert np.all(np.isfinite(th1)) and not np.array_equal(th1, th0)
