"""Learned per-parameter inner step sizes (trainable_inner_step_size, promp_set_train_step_sizes), shared by
test_emu_step_sizes.py (emulator, tiny) and test_gpu_step_sizes.py (MI355X).

Per task the inner chain is theta_{k+1} = theta_k - alpha * g_k; with lam_k = dJ/dtheta_k of the backward sweep the objective's
gradient with respect to alpha is (1/M) sum_i sum_k -lam_{k+1} * g_k.  Two float64 references, independent of each other:

  (a) analytic: the chain walked as oracle.promp.meta_objective_and_grad / oracle.dice.meta_objective_and_grad walk it
      (loss_and_grad, hvp), accumulating -lam_{k+1} * g_k;
  (b) central differences in alpha (step 1e-5, fourth-order stencil: central_differences says why) of the objective's VALUE at
      32 seeded coordinates plus every log_std coordinate.

(b) for the DiCE inner objective.  The magic box exp(tau - stop_gradient(tau)) has the value one: oracle.dice's loss is the
constant -mean(R m), and the Jacobian of oracle.dice's gradient FUNCTION is the log-likelihood Hessian alone -- the path-coupled
second-order term the meta-gradient carries (oracle.dice.hvp, autograd through the box) is the derivative with respect to the
box's live argument only.  A finite difference therefore has to hold the stop_gradient side where autograd holds it: at the
unperturbed chain.  dice_frozen_objective evaluates F(theta, ref) = -(1/N) sum R m exp(tau(theta) - tau(ref)) that way (inner
steps by d/dtheta F, the outer value by F itself); at the unperturbed alpha it IS oracle.dice's loss and oracle.dice's chain,
which check_references asserts before anything is differenced.

Inputs: alpha seeded in [0.02, 0.2] and non-uniform, two entries exactly 0 (nothing may divide by alpha), eta = helpers.eta_for(K):
5e-4, 1e-3, doubling on, clip 0.3.  Tolerance: the project's own for a meta-gradient against the float64 oracle, rel_max < 1e-4; (a) against (b): 1e-7.
"""
import numpy as np
import pytest

from oracle import dice, policy as op, promp as pm
from promp_amd import _lib
from tests import dice_shape_checks as ds, helpers
from tests.parity_checks import assert_adam_trajectory, make_ctx, rel_max, upload_dice_slabs

TOL = 1e-4
REF_TOL = 1e-7
CLIP = 0.3
FD_STEP = 1e-5


def eta_for(K):
    return helpers.eta_for(K)


def fd_coords(seed, n, A):
    """32 seeded coordinates outside log_std, then every log_std coordinate"""
    rng = np.random.RandomState(seed + 4242)
    return np.concatenate([np.sort(rng.choice(n - A, 32, replace=False)), np.arange(n - A, n)])


def make_alpha(seed, n, A):
    """seeded in [0.02, 0.2]; the first two finite-difference coordinates are exactly 0"""
    rng = np.random.RandomState(seed + 77)
    a = rng.uniform(0.02, 0.2, n).astype(np.float32)
    a[fd_coords(seed, n, A)[:2]] = 0.0
    return a


# ---- (a) analytic ------------------------------------------------------------------------------------------------------

def analytic(spec, theta, all_slabs, alpha, eta, inner_kind=pm.INNER_RATIO, outer_kind=pm.OUTER_CLIP, dice_outer=None):
    """-> dict(grad, grad_alpha, loss): oracle.promp.meta_objective_and_grad's walk (promp.py:199-216) -- dice_outer in
    ('dice', 'vpg'): oracle.dice.meta_objective_and_grad's -- with -lam_{k+1} * g_k accumulated on the way back"""
    K, M = len(all_slabs) - 1, len(all_slabs[0])
    theta, alpha = np.asarray(theta, np.float64), np.asarray(alpha, np.float64)
    g_th, g_al = np.zeros_like(theta), np.zeros_like(theta)
    for i in range(M):
        thetas, gs, gkls = [theta], [], []
        for k in range(K):
            sl = all_slabs[k][i]
            if dice_outer:
                gs.append(dice.loss_and_grad(spec, thetas[k], sl, k == 0)['grad'])
                gkls.append(0.0)
            else:
                r = pm.loss_and_grad(spec, thetas[k], sl, inner_kind, clip_log_std=(k == 0))
                gs.append(r['grad'])
                gkls.append(r['grad_kl'])
            thetas.append(thetas[k] - alpha * gs[k])
        last = all_slabs[K][i]
        if dice_outer == 'dice':
            lam = dice.loss_and_grad(spec, thetas[K], last, False)['grad']
        elif dice_outer == 'vpg':
            lam = pm.loss_and_grad(spec, thetas[K], dict(last, advantages=last['vpg_advantages']), 'loglik', False)['grad']
        else:
            lam = pm.loss_and_grad(spec, thetas[K], last, outer_kind, clip_log_std=False, clip_eps=CLIP)['grad']
        for k in range(K - 1, -1, -1):
            g_al -= lam * gs[k]
            if dice_outer:
                lam = lam - dice.hvp(spec, thetas[k], all_slabs[k][i], alpha * lam, k == 0)
            else:
                lam = lam - pm.hvp(spec, thetas[k], all_slabs[k][i], alpha * lam, inner_kind, clip_log_std=(k == 0)) \
                    + (eta[k] / K) * gkls[k]
        g_th += lam
    return dict(grad=g_th / M, grad_alpha=g_al / M)


# ---- (b) central differences -------------------------------------------------------------------------------------------

def central_differences(f, alpha, coords, h=FD_STEP):
    """Central differences of f in alpha_j at step h, fourth order: (8 [f(+h) - f(-h)] - [f(+2h) - f(-2h)]) / 12h.
    The two-point form's truncation error h^2 f(3) / 6 is not small here: a log_std step size moves sigma exponentially, and at
    the GPU file's DiCE shape the two-point quotient at h = 1e-5 is 4.0e-5 (relative) off the analytic value -- 4.0e-3 at 1e-4,
    4.1e-7 at 1e-6, i.e. h^2 to three digits, the reference's own error and 400 times the 1e-7 the two references are held to.
    The second pair of evaluations cancels that term at the same step."""
    alpha = np.asarray(alpha, np.float64)
    out = np.zeros(len(coords))

    def diff(j, step):
        ap, am = alpha.copy(), alpha.copy()
        ap[j] += step
        am[j] -= step
        return f(ap) - f(am)
    for n, j in enumerate(coords):
        out[n] = (8.0 * diff(j, h) - diff(j, 2.0 * h)) / (12.0 * h)
    return out


def promp_objective(spec, theta, all_slabs, eta, inner_kind=pm.INNER_RATIO, outer_kind=pm.OUTER_CLIP):
    return lambda a: pm.meta_objective_and_grad(spec, theta, all_slabs, a, eta, CLIP, inner_kind, outer_kind, want_grad=False)['loss']


def _row_logp(spec, theta, slab, clip_log_std):
    obs = np.asarray(slab['observations'], dtype=np.float64)
    act = np.asarray(slab['actions'], dtype=np.float64)
    mu, s, _ = op.forward(spec, theta, obs, clip_log_std)
    z = (act - mu) * np.exp(-s)
    return -np.sum(s) - 0.5 * np.sum(z ** 2, axis=1) - 0.5 * act.shape[1] * np.log(2.0 * np.pi)


def _box(spec, theta, ref, slab, clip_log_std):
    """exp(tau(theta) - tau(ref)) per row, tau the cumulative log-likelihood within the row's path"""
    d = _row_logp(spec, theta, slab, clip_log_std) - _row_logp(spec, ref, slab, clip_log_std)
    off = slab['path_row_offsets']
    return np.exp(np.concatenate([np.cumsum(d[off[p]:off[p + 1]]) for p in range(len(off) - 1)]))


def _frozen_value(spec, theta, ref, slab, clip_log_std):
    return -float(np.sum(slab['dice_rw'] * _box(spec, theta, ref, slab, clip_log_std))) / len(slab['dice_rw'])


def _frozen_grad(spec, theta, ref, slab, clip_log_std):
    """d/dtheta of _frozen_value: the log-likelihood gradient with the suffix sums of R m box as weights"""
    rb = slab['dice_rw'] * _box(spec, theta, ref, slab, clip_log_std)
    off = slab['path_row_offsets']
    w = np.concatenate([np.cumsum(rb[off[p]:off[p + 1]][::-1])[::-1] for p in range(len(off) - 1)])
    return pm.loss_and_grad(spec, theta, dict(slab, advantages=w), 'loglik', clip_log_std)['grad']


def dice_frozen_objective(spec, theta, all_slabs, alpha0, outer='dice'):
    """-> f(alpha): DICEMAML's meta-objective with every stop_gradient held at the chain of alpha0 (see the module docstring)"""
    K, M = len(all_slabs) - 1, len(all_slabs[0])
    theta = np.asarray(theta, np.float64)
    refs = dice.meta_objective_and_grad(spec, theta, all_slabs, np.asarray(alpha0, np.float64), want_grad=False, outer=outer)
    chains = []
    for i in range(M):
        ch = [theta]
        for k in range(K):
            ch.append(ch[k] - alpha0 * dice.loss_and_grad(spec, ch[k], all_slabs[k][i], k == 0)['grad'])
        assert np.array_equal(ch[K], refs['adapted'][i])
        chains.append(ch)

    def f(a):
        tot = 0.0
        for i in range(M):
            th = theta
            for k in range(K):
                th = th - a * _frozen_grad(spec, th, chains[i][k], all_slabs[k][i], k == 0)
            last = all_slabs[K][i]
            if outer == 'vpg':
                tot += pm.loss_and_grad(spec, th, dict(last, advantages=last['vpg_advantages']), 'loglik', False, want_grad=False)['loss']
            else:
                tot += _frozen_value(spec, th, chains[i][K], last, False)
        return tot / M
    f.loss0 = refs['loss']
    return f


# ---- cases -------------------------------------------------------------------------------------------------------------

class PrompCase(object):
    def __init__(self, seed, M, P, T, O, A, hidden, K, ragged=False):
        self.seed, self.M, self.O, self.A, self.hidden, self.K = seed, M, O, A, tuple(hidden), K
        self.theta, self.all_slabs, self.all_paths = helpers.make_promp_case(seed, M, P, T, O, A, hidden, K, ragged=ragged)
        self.spec = op.PolicySpec(O, A, hidden)
        self.n = self.spec.n_params
        self.alpha = make_alpha(seed, self.n, A)
        self.eta = eta_for(K)
        self.coords = fd_coords(seed, self.n, A)
        self.t64, self.a64, self.e64 = self.theta.astype(np.float64), self.alpha.astype(np.float64), self.eta.astype(np.float64)
        self._ref = None

    def ref(self):
        if self._ref is None:
            self._ref = analytic(self.spec, self.t64, self.all_slabs, self.a64, self.e64)
        return self._ref

    def fd(self):
        return central_differences(promp_objective(self.spec, self.t64, self.all_slabs, self.e64), self.a64, self.coords)

    def ctx(self, lib):
        ctx = make_ctx(lib, self.M, self.O, self.A, self.hidden, self.K, self.all_paths)
        helpers.upload_slabs(ctx, self.all_paths, self.all_slabs)
        ctx.set_theta(self.theta)
        ctx.set_step_sizes(self.alpha)
        return ctx


def check_references(case):
    """(a) against (b) where both exist, and (a)'s theta-gradient against the oracle's own: float64, no device"""
    r = case.ref()
    g = pm.meta_objective_and_grad(case.spec, case.t64, case.all_slabs, case.a64, case.e64, CLIP)['grad']
    assert rel_max(r['grad'], g) < 1e-12
    fd = case.fd()
    err = rel_max(r['grad_alpha'][case.coords], fd)
    print('analytic vs central differences: rel_max %.3e' % err)
    assert err < REF_TOL
    assert np.all(case.a64[case.coords[:2]] == 0.0) and np.all(fd[:2] != 0.0)      # a zero step size still has a gradient


def check_dice_references(c, outer='dice'):
    theta, _, all_slabs = ds.make_case(c)
    spec = op.PolicySpec(c['O'], c['A'], c['hidden'])
    alpha = make_alpha(c['seed'], spec.n_params, c['A']).astype(np.float64)
    coords = fd_coords(c['seed'], spec.n_params, c['A'])
    r = analytic(spec, theta, all_slabs, alpha, np.zeros(c['K']), dice_outer=outer)
    g = dice.meta_objective_and_grad(spec, theta, all_slabs, alpha, outer=outer)
    assert rel_max(r['grad'], g['grad']) < 1e-12
    f = dice_frozen_objective(spec, theta, all_slabs, alpha, outer)
    assert abs(f(alpha) - g['loss']) <= 1e-12 * max(1.0, abs(g['loss']))         # the frozen form IS oracle.dice's loss at alpha
    fd = central_differences(f, alpha, coords)
    err = rel_max(r['grad_alpha'][coords], fd)
    print('DiCE (%s outer) analytic vs central differences: rel_max %.3e' % (outer, err))
    assert err < REF_TOL
    # and the log-likelihood Hessian alone (what differencing oracle.dice's own gradient function would give) is not it
    if c['K'] > 1:
        plain = analytic(spec, theta, [[dict(sl) for sl in step] for step in all_slabs], alpha, np.zeros(c['K']),
                         inner_kind='loglik', outer_kind='loglik')['grad_alpha']
        assert rel_max(plain[coords], fd) > 100 * REF_TOL
    return spec, theta, all_slabs, alpha, coords, r, fd


# ---- device checks -----------------------------------------------------------------------------------------------------

def check_alpha_grad(lib, case, schedule=None):
    """promp_meta_grad with the flag on: the step-size gradient against (a) and (b); the theta-gradient, the statistics and the
    exchange length with the flag off / on.  -> the device's step-size gradient"""
    ctx = case.ctx(lib)
    if schedule is not None:
        ctx.set_schedule(fuse_min_tasks=schedule)
    n, K = case.n, case.K
    assert ctx.reduced_count() == n + K + 2
    g_off, st_off = ctx.meta_grad(CLIP, case.eta)
    red_off = ctx.reduced_get()
    ctx.set_train_step_sizes(True)
    assert ctx.reduced_count() == 2 * n + K + 2
    g_on, st_on = ctx.meta_grad(CLIP, case.eta)
    ga = ctx.get_step_size_grad()
    red_on = ctx.reduced_get()
    assert np.array_equal(g_on, g_off)
    for key in ('loss', 'inner_kl', 'outer_kl'):
        assert np.array_equal(st_on[key], st_off[key]), key
    assert red_on.shape == (2 * n + K + 2,) and np.array_equal(red_on[:n + K + 2], red_off)
    assert np.array_equal(ctx.get_step_sizes(), case.alpha)                           # a gradient evaluation moves nothing
    r = case.ref()
    e_a, e_b = rel_max(ga, r['grad_alpha']), rel_max(ga[case.coords], case.fd())
    print('step-size gradient: rel_max %.3e vs analytic, %.3e vs central differences' % (e_a, e_b))
    assert rel_max(g_on, r['grad']) < TOL
    assert e_a < TOL and e_b < TOL
    # the task sums the exchange carries are the mean times M (single rank: M_global = M)
    assert rel_max(red_on[n + K + 2:] / case.M, r['grad_alpha']) < TOL
    ctx.set_train_step_sizes(False)                                                   # off again means off again
    assert ctx.reduced_count() == n + K + 2
    g2, _ = ctx.meta_grad(CLIP, case.eta)
    assert np.array_equal(g2, g_off)
    ctx.close()
    return ga


def check_dice_alpha_grad(lib, c):
    """PROMP_INNER_DICE: lam must be complete -- both pieces of the R-operator reduction of step k + 1 -- when step k's product
    with g_k is taken: against (b), and against (a)"""
    spec, theta, all_slabs, alpha, coords, r, fd = check_dice_references(c)
    M, K, n = c['M'], c['K'], spec.n_params
    R = max(sum(len(sl['dice_rw']) for sl in step) for step in all_slabs)
    NPaths = max(sum(len(sl['path_row_offsets']) - 1 for sl in step) for step in all_slabs)
    ctx = _lib.Context(M, c['O'], c['A'], c['hidden'], K, max_rows=R, max_paths=NPaths, lib=lib)
    upload_dice_slabs(ctx, all_slabs)
    ctx.set_theta(theta.astype(np.float32))
    ctx.set_step_sizes(alpha.astype(np.float32))
    eta0 = np.zeros(K, np.float32)
    g_off, _ = ctx.meta_grad(0.0, eta0, _lib.INNER_DICE, _lib.OUTER_LOGLIK)
    ctx.set_train_step_sizes(True)
    g_on, _ = ctx.meta_grad(0.0, eta0, _lib.INNER_DICE, _lib.OUTER_LOGLIK)
    ga = ctx.get_step_size_grad()
    ctx.close()
    assert np.array_equal(g_on, g_off)
    assert rel_max(g_on, r['grad']) < TOL
    e_a, e_b = rel_max(ga, r['grad_alpha']), rel_max(ga[coords], fd)
    print('DiCE step-size gradient: rel_max %.3e vs analytic, %.3e vs central differences' % (e_a, e_b))
    assert e_b < TOL and e_a < TOL


def check_learn_std_false(lib, case, epochs=2):
    """learn_std = False: the trailing A step sizes are exactly 0 and stay so, their Adam slots and reported gradient too"""
    A = case.A
    ctx = case.ctx(lib)
    ctx.set_learn_std(False)
    ctx.set_train_step_sizes(True)
    th0 = ctx.get_theta()
    assert np.all(ctx.get_step_sizes()[-A:] == 0.0)
    ctx.optimize(epochs, 1e-3, CLIP, case.eta)
    ctx.meta_grad(CLIP, case.eta)
    s, ga = ctx.get_step_sizes(), ctx.get_step_size_grad()
    m, v = ctx.get_step_size_adam_state()
    assert np.all(s[-A:] == 0.0) and np.all(ga[-A:] == 0.0) and np.all(m[-A:] == 0.0) and np.all(v[-A:] == 0.0)
    assert np.array_equal(ctx.get_theta()[-A:], th0[-A:])
    assert np.all(np.isfinite(s)) and np.mean(s[:-A] != case.alpha[:-A]) > 0.9       # the others are trained
    ctx.close()


def check_adam(lib, case, epochs=3, lr=1e-3):
    """E epochs of Adam on theta AND alpha against the float64 loop (oracle gradients, oracle.promp.adam_step on each), per
    element as parity_checks.check_meta holds theta's trajectory; the slots' accessors round-trip exactly"""
    ctx = case.ctx(lib)
    ctx.set_train_step_sizes(True)
    v0 = ctx.state_version()
    ctx.optimize(epochs, lr, CLIP, case.eta)
    assert ctx.state_version() > v0
    th_e, al_e = case.t64.copy(), case.a64.copy()
    st_t, st_a = pm.AdamState(case.n), pm.AdamState(case.n)
    tmin = amin = None
    tmax, amax = [], []
    for _ in range(epochs):
        r = analytic(case.spec, th_e, case.all_slabs, al_e, case.e64)
        gt, ga = r['grad'], r['grad_alpha']
        tmin = np.abs(gt) if tmin is None else np.minimum(tmin, np.abs(gt))
        amin = np.abs(ga) if amin is None else np.minimum(amin, np.abs(ga))
        tmax.append(np.max(np.abs(gt)))
        amax.append(np.max(np.abs(ga)))
        th_e = pm.adam_step(th_e, gt, st_t, lr)
        al_e = pm.adam_step(al_e, ga, st_a, lr)
    m, v, t = ctx.get_adam_state()
    am, av = ctx.get_step_size_adam_state()
    assert t == epochs
    assert_adam_trajectory(ctx.get_theta().astype(np.float64) - case.t64, th_e - case.t64, tmin, np.array(tmax), lr, epochs,
                           m_dev=m, v_dev=v, m_ref=st_t.m, v_ref=st_t.v)
    worst, excluded = assert_adam_trajectory(ctx.get_step_sizes().astype(np.float64) - case.a64, al_e - case.a64, amin,
                                             np.array(amax), lr, epochs, m_dev=am, v_dev=av, m_ref=st_a.m, v_ref=st_a.v)
    print('alpha after %d epochs: worst judged entry %.3e of one step, %.1f %% below the gradient floor' % (epochs, worst, 100 * excluded))
    # round trip
    rng = np.random.RandomState(case.seed + 5)
    m2, v2 = rng.randn(case.n).astype(np.float32), rng.rand(case.n).astype(np.float32)
    ctx.set_step_size_adam_state(m2, v2)
    m3, v3 = ctx.get_step_size_adam_state()
    assert np.array_equal(m2, m3) and np.array_equal(v2, v3)
    ctx.close()


def _state(ctx):
    m, v, t = ctx.get_adam_state()
    am, av = ctx.get_step_size_adam_state()
    return dict(theta=ctx.get_theta(), alpha=ctx.get_step_sizes(), m=m, v=v, am=am, av=av, t=t)


def _assert_same_state(a, b):
    for key in ('theta', 'alpha', 'm', 'v', 'am', 'av'):
        assert np.array_equal(a[key], b[key]), key
    assert a['t'] == b['t']


def check_split_equals_fused(lib, case, epochs=2):
    """k_reduce_final -> [exchange] -> k_mean_adam against k_final_adam with the step sizes' columns: forced split path, a
    one-rank communicator (all-reduce of 2 Theta + K + 2 floats), the fixed-order exchange"""
    def run(split=False, comm=False, fixed=False):
        ctx = case.ctx(lib)
        ctx.set_train_step_sizes(True)
        if comm:
            ctx.comm_init(0, 1, _lib.comm_unique_id(lib))
            ctx.comm_fixed_order(fixed)
        if split:
            ctx.comm_split_path(True)
        ctx.optimize(epochs, 1e-3, CLIP, case.eta)
        g, _ = ctx.meta_grad(CLIP, case.eta)
        out = dict(_state(ctx), g=g, ga=ctx.get_step_size_grad(), red=ctx.reduced_get())
        ctx.close()
        return out
    fused = run()
    assert not np.array_equal(fused['alpha'], case.alpha)
    for kw in (dict(split=True), dict(split=True, comm=True), dict(split=True, comm=True, fixed=True)):
        other = run(**kw)
        _assert_same_state(fused, other)
        for key in ('g', 'ga', 'red'):
            assert np.array_equal(fused[key], other[key]), (kw, key)


def check_host_exchange_route(lib, case, epochs=2):
    """The caller's own exchange with the flag on (promp_meta_grad -> promp_reduced_get -> promp_reduced_set -> promp_adam_step: what
    DeviceSession.optimize runs under a `collective`) against promp_optimize, bit for bit; promp_adam_step refuses an exchange
    buffer that holds no step-size sums instead of stepping on zeros or on stale columns"""
    ctx = case.ctx(lib)
    ctx.set_train_step_sizes(True)
    ctx.optimize(epochs, 1e-3, CLIP, case.eta)
    fused = _state(ctx)
    ctx.close()
    ctx = case.ctx(lib)
    ctx.meta_grad(CLIP, case.eta)                       # flag off: [Theta | K + 2] only
    ctx.set_train_step_sizes(True)
    with pytest.raises(_lib.PrompError, match='no step-size gradient'):
        ctx.adam_step(1e-3)
    for _ in range(epochs):
        ctx.meta_grad(CLIP, case.eta)
        red = ctx.reduced_get()
        assert red.shape == (2 * case.n + case.K + 2,)
        ctx.reduced_set(red.copy())
        ctx.adam_step(1e-3)
    _assert_same_state(fused, _state(ctx))
    ctx.constraint_hvp(np.ones(case.n, np.float32), _lib.INNER_RATIO)       # leaves the step sizes' columns stale
    with pytest.raises(_lib.PrompError, match='no step-size gradient'):
        ctx.adam_step(1e-3)
    _assert_same_state(fused, _state(ctx))                                  # a refused step moved nothing, the step count included
    ctx.close()


def check_reuse_adapt(lib, case, epochs=2):
    """promp_inner_adapt leaves g_0 behind: the first epoch skips its inner pass with the flag on too, bit for bit"""
    def run(reuse):
        ctx = case.ctx(lib)
        ctx.set_reuse_adapt(reuse)
        ctx.set_train_step_sizes(True)
        ctx.switch_to_pre_update()
        ctx.inner_adapt(0)
        ctx.optimize(epochs, 1e-3, CLIP, case.eta)
        out = (_state(ctx), ctx.adapt_passes_skipped())
        # the step sizes have moved: the pass promp_inner_adapt left behind no longer stands
        ctx.switch_to_pre_update()
        ctx.inner_adapt(0)
        tt = ctx.get_task_thetas()
        ctx.close()
        return out + (tt,)
    off, on = run(False), run(True)
    _assert_same_state(off[0], on[0])
    assert off[1] == 0 and on[1] > 0, (off[1], on[1])
    assert np.array_equal(off[2], on[2])
    assert not np.array_equal(on[0]['alpha'], case.alpha)


def check_schedule_invariance(lib, case):
    """fuse_min_tasks = 1 (the chain kernels reduce R-operator passes in-launch) against the default: same bits"""
    ga_default = check_alpha_grad(lib, case)
    ga_fused = check_alpha_grad(lib, case, schedule=1)
    assert np.array_equal(ga_default, ga_fused)


# ---- plugin level --------------------------------------------------------------------------------------------------------

def build_trainer(algo_name, trainable, n_itr, log_dir=None, inner_lr=0.1):
    """Trainer on the point environment with device rollouts, (32, 32) policy: ProMP / VPGMAML / DICEMAML"""
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
    common = dict(policy=policy, inner_lr=inner_lr, meta_batch_size=M, num_inner_grad_steps=1, trainable_inner_step_size=trainable)
    if algo_name == 'dice':
        proc = DiceMetaSampleProcessor(baseline=LinearTimeBaseline(), max_path_length=T, discount=0.99, normalize_adv=True)
        algo = DICEMAML(T, learning_rate=1e-3, **common)
    else:
        proc = MetaSampleProcessor(baseline=LinearFeatureBaseline(), discount=0.99, gae_lambda=1, normalize_adv=True)
        algo = (VPGMAML(learning_rate=1e-3, **common) if algo_name == 'vpg' else
                ProMP(learning_rate=1e-3, num_ppo_steps=2, clip_eps=0.3, init_inner_kl_penalty=5e-4, adaptive_inner_kl_penalty=False, **common))
    return Trainer(algo=algo, policy=policy, env=env, sampler=sampler, sample_processor=proc, n_itr=n_itr, num_inner_grad_steps=1)


LOG_KEYS = ('InnerStepSize-Mean', 'InnerStepSize-Min', 'InnerStepSize-Max')


def train_and_grab(trainer):
    from promp_amd.utils import logger
    seen, orig = {}, logger.dumpkvs

    def grab():
        seen.update(logger.getkvs())
        return orig()
    logger.dumpkvs = grab
    try:
        trainer.train()
    finally:
        logger.dumpkvs = orig
    return seen


def check_plugin(algo_name, n_itr, tmp_dir=None):
    """trainable_inner_step_size through Trainer: True trains and logs the step sizes, False leaves np.full(Theta, inner_lr)"""
    trainer = build_trainer(algo_name, True, n_itr, log_dir=tmp_dir)
    n = trainer.policy.session.theta.size
    lr0 = np.full(n, 0.1, np.float32)
    assert np.array_equal(trainer.algo.step_sizes, lr0)
    seen = train_and_grab(trainer)
    s = trainer.algo.step_sizes
    assert s.shape == (n,) and np.all(np.isfinite(s)) and np.mean(s != lr0) > 0.5
    for k in LOG_KEYS:
        assert k in seen, k
    assert seen['InnerStepSize-Min'] <= seen['InnerStepSize-Mean'] <= seen['InnerStepSize-Max']
    off = build_trainer(algo_name, False, n_itr)
    seen_off = train_and_grab(off)
    assert np.array_equal(off.algo.step_sizes, lr0)
    assert not any(k in seen_off for k in LOG_KEYS)
    return trainer


def check_snapshot_round_trip(trainer, path):
    """a snapshot restores the trained step sizes and their Adam slots exactly; one without them loads as before"""
    from promp_amd.utils import logger
    snap = logger.load_params(path)
    sess = trainer.policy.session
    assert np.array_equal(snap['inner_step_sizes'], trainer.algo.step_sizes)
    am, av = sess.ctx.get_step_size_adam_state()
    assert np.array_equal(snap['step_adam_m'], am) and np.array_equal(snap['step_adam_v'], av) and np.any(am != 0.0)
    again = build_trainer('promp', True, 4)
    again.load_snapshot(path)
    assert again.start_itr == snap['itr'] + 1
    ctx = again.policy.session.ensure()
    assert np.array_equal(again.algo.step_sizes, snap['inner_step_sizes'])
    am2, av2 = ctx.get_step_size_adam_state()
    assert np.array_equal(am2, am) and np.array_equal(av2, av)
    # a re-created context (more rows than it was sized for) carries the flag, the step sizes and the slots along
    again.policy.session.ensure(rows=10 * again.policy.session.capacity[0] + 1000)
    assert again.policy.session.ctx is not ctx
    assert np.array_equal(again.algo.step_sizes, snap['inner_step_sizes'])
    am3, av3 = again.policy.session.ctx.get_step_size_adam_state()
    assert np.array_equal(am3, am) and np.array_equal(av3, av)
    old = {k: v for k, v in snap.items() if k not in ('inner_step_sizes', 'step_adam_m', 'step_adam_v')}
    plain = build_trainer('promp', False, 4)
    with pytest.raises(ValueError, match='trainable_inner_step_size'):       # trained step sizes into a run that cannot train them
        plain.load_snapshot(snap)
    plain.load_snapshot(old)
    assert np.array_equal(plain.algo.step_sizes, np.full(snap['inner_step_sizes'].size, 0.1, np.float32))


def check_memo_key():
    """ADVICE: algo.optimizer.loss() after session.set_step_sizes re-evaluates instead of answering from the memo"""
    from promp_amd.meta_algos.pro_mp import ProMP
    from promp_amd.policies.meta_gaussian_mlp_policy import MetaGaussianMLPPolicy
    from promp_amd.utils import logger
    logger.configure(quiet=True)
    M, O, A, hidden = 2, 5, 3, (32, 32)
    theta, all_slabs, _ = helpers.make_promp_case(57, M, 2, 20, O, A, hidden, 1)
    spec = op.PolicySpec(O, A, hidden)
    policy = MetaGaussianMLPPolicy(name='p', obs_dim=O, action_dim=A, meta_batch_size=M, hidden_sizes=hidden)
    policy.set_params(spec.to_ordered_dict(theta))
    algo = ProMP(policy=policy, inner_lr=0.1, meta_batch_size=M, num_inner_grad_steps=1, learning_rate=1e-3, num_ppo_steps=1, clip_eps=0.3,
                 init_inner_kl_penalty=5e-4, adaptive_inner_kl_penalty=False)
    samples = [[dict(observations=s['observations'], actions=s['actions'], advantages=s['advantages'], agent_infos=s['agent_infos'])
                for s in step] for step in all_slabs]
    algo.optimize_policy(samples, log=False)
    l0 = algo.optimizer.loss(samples)
    assert l0 == algo.last_stats['loss_after']                 # (answered from what the optimisation handed back)
    assert algo.optimizer.loss(samples) == l0
    algo.session.set_step_sizes(np.full(spec.n_params, 0.3, np.float32))
    l1 = algo.optimizer.loss(samples)
    th = spec.from_ordered_dict(policy.get_param_values()).astype(np.float64)
    ref = pm.meta_objective_and_grad(spec, th, all_slabs, np.full(spec.n_params, 0.3), np.array([5e-4]), CLIP, want_grad=False)['loss']
    assert l1 != l0
    np.testing.assert_allclose(l1, ref, rtol=1e-4, atol=1e-6)
