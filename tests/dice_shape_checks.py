"""DiCE objectives (PROMP_INNER_DICE) on every pass-kernel family, shared by test_emu_dice_shapes.py (emulator, tiny) and
test_gpu_dice_shapes.py (MI355X): what parity_checks.check_dice / check_vpg_dice run, on inputs generated here instead of the
committed fixtures (those hold register-chained shapes only).

References (float64): oracle.dice (adapt, meta_objective_and_grad) and, independently, torch.autograd on the padded magic-box
graph (oracle.gen_golden.torch_dice_meta_objective).  oracle.dice.row_tangent assumes tanh hidden layers and a linear output;
for every other activation the reference is torch_dice_general below, the same graph with the activations as parameters,
pinned against oracle.dice on a tanh case by the test files before it is used.

Tolerance: the project's own for a meta-gradient against the float64 oracle, rel_max < 1e-4 (parity_checks.check_dice).
"""
import numpy as np

from oracle import dice, gen_golden as gg, policy as op
from promp_amd import _lib
from tests.parity_checks import rel_max, upload_dice_slabs

TOL = 1e-4


def case(seed, M, P, T, O, A, hidden, K=1, alpha=0.1, ragged=False, Tmax=None, trim=()):
    """trim: (step, task, path, length) entries that cut a path short (mask zero from `length` on) -- path lengths chosen by
    the test: a path of one row, a task whose row count leaves a partial last tile"""
    return dict(seed=seed, M=M, P=P, T=T, Tmax=Tmax or T, O=O, A=A, hidden=tuple(hidden), K=K, alpha=alpha, ragged=ragged,
                trim=tuple(trim))


def make_case(c):
    """-> theta float64, padded samples [K+1][M] (with 'advantages' on the last step, for the VPG-DiCE outer objective),
    flat slabs [K+1][M] (oracle.dice.to_slab)"""
    theta, all_samples = gg.make_dice_inputs(c)
    for (k, i, p, n) in c['trim']:
        all_samples[k][i]['mask'][p, n:] = 0.0
    rng = np.random.RandomState(c['seed'] + 1000)
    for sd in all_samples[c['K']]:
        sd['advantages'] = rng.randn(*sd['mask'].shape)
    all_slabs = [[dice.to_slab(sd) for sd in step] for step in all_samples]
    return theta.astype(np.float64), all_samples, all_slabs


def task_rows(all_slabs, k=0):
    return [len(sl['dice_rw']) for sl in all_slabs[k]]


def path_lengths(all_slabs, k=0):
    return np.concatenate([np.diff(sl['path_row_offsets']) for sl in all_slabs[k]])


def torch_dice_general(theta, all_samples, c, hidden_act='tanh', output_act='identity', outer='dice', min_log_std=float(np.log(1e-6))):
    """DICEMAML.build_graph's forward arithmetic on the padded [P, Tmax] arrays in torch float64 (cumulative log-likelihoods,
    magic box, mask; K inner steps with create_graph), hidden and output nonlinearity as parameters.  -> loss, gradient,
    adapted parameters [M][Theta]"""
    import torch
    O, A, hidden = c['O'], c['A'], c['hidden']
    sizes = (O,) + tuple(hidden) + (A,)
    f = dict(tanh=torch.tanh, relu=torch.relu, identity=lambda x: x)
    th = torch.tensor(np.asarray(theta, dtype=np.float64), requires_grad=True)
    T = lambda x: torch.tensor(np.asarray(x, dtype=np.float64))

    def obj(t, sd, clip, vpg):
        P_, Tm = sd['mask'].shape
        x, off = T(sd['observations']).reshape(P_ * Tm, O), 0
        for i in range(len(sizes) - 1):
            W = t[off:off + sizes[i] * sizes[i + 1]].reshape(sizes[i], sizes[i + 1]); off += sizes[i] * sizes[i + 1]
            b = t[off:off + sizes[i + 1]]; off += sizes[i + 1]
            x = f[hidden_act if i < len(sizes) - 2 else output_act](x @ W + b)
        s = t[off:off + A]
        if clip:
            s = torch.maximum(s, torch.tensor(min_log_std, dtype=torch.float64))
        z = (T(sd['actions']).reshape(P_ * Tm, A) - x) * torch.exp(-s)
        ll = (-s.sum() - 0.5 * (z ** 2).sum(-1) - 0.5 * A * np.log(2 * np.pi)).reshape(P_, Tm)
        if vpg:
            return -(ll * T(sd['advantages']) * T(sd['mask'])).mean()
        tau = torch.cumsum(ll, dim=1)
        return -(torch.exp(tau - tau.detach()) * T(sd['adjusted_rewards']) * T(sd['mask'])).mean()

    objs, adapted = [], []
    for i in range(c['M']):
        cur, clip = th, True
        for k in range(c['K']):
            g, = torch.autograd.grad(obj(cur, all_samples[k][i], clip, False), cur, create_graph=True)
            cur, clip = cur - c['alpha'] * g, False
        adapted.append(cur.detach().numpy())
        objs.append(obj(cur, all_samples[c['K']][i], False, outer == 'vpg'))
    loss = torch.stack(objs).mean()
    grad, = torch.autograd.grad(loss, th)
    return float(loss.detach()), grad.numpy(), adapted


def check_general_reference_against_oracle(c):
    """torch_dice_general with tanh hidden layers and a linear output IS oracle.dice's objective: both outer objectives"""
    t64, all_samples, all_slabs = make_case(c)
    spec = op.PolicySpec(c['O'], c['A'], c['hidden'])
    alpha = np.full(spec.n_params, c['alpha'])
    for outer in ('dice', 'vpg'):
        loss, grad, adapted = torch_dice_general(t64, all_samples, c, outer=outer)
        r = dice.meta_objective_and_grad(spec, t64, all_slabs, alpha, outer=outer)
        np.testing.assert_allclose(loss, r['loss'], rtol=1e-10, atol=1e-12)
        assert rel_max(grad, r['grad']) < 1e-9
        assert rel_max(np.stack(adapted), np.stack(r['adapted'])) < 1e-10


def references(c, t64, all_samples, all_slabs, hidden_act, output_act):
    """-> {outer: [(name, loss, grad), ...]}, adapted parameters after the FIRST inner step [M][Theta]"""
    out_act = output_act or 'identity'
    spec = op.PolicySpec(c['O'], c['A'], c['hidden'], hidden_act=hidden_act, output_act=out_act)
    alpha = np.full(spec.n_params, c['alpha'])
    refs = {}
    if hidden_act == 'tanh' and out_act == 'identity':
        for outer in ('dice', 'vpg'):
            r = dice.meta_objective_and_grad(spec, t64, all_slabs, alpha, outer=outer)
            tl, tg = gg.torch_dice_meta_objective(t64, all_samples, c, outer=outer)
            refs[outer] = [('oracle', r['loss'], r['grad']), ('torch', tl, tg)]
    else:
        for outer in ('dice', 'vpg'):
            tl, tg, _ = torch_dice_general(t64, all_samples, c, hidden_act, out_act, outer=outer)
            refs[outer] = [('torch', tl, tg)]
    # (the inner step is a first-order quantity: oracle.dice.adapt holds for every activation)
    return refs, np.stack(dice.adapt(spec, [t64] * c['M'], all_slabs[0], alpha))


def check_dice_shape(lib, c, hidden_act='tanh', output_act=None, tol=TOL, verbose=True):
    """One case through the C ABI: inner step, exact DICE-MAML meta-gradient (and that the coupling term matters), exact
    VPG-DiCE-MAML meta-gradient (and that the outer objective matters).  -> the DICE-MAML meta-gradient as the device gave it"""
    t64, all_samples, all_slabs = make_case(c)
    refs, ad = references(c, t64, all_samples, all_slabs, hidden_act, output_act)
    M, K = c['M'], c['K']
    R = max(sum(task_rows(all_slabs, k)) for k in range(K + 1))
    NPaths = max(len(path_lengths(all_slabs, k)) for k in range(K + 1))
    ctx = _lib.Context(M, c['O'], c['A'], c['hidden'], K, max_rows=R, max_paths=NPaths, lib=lib, hidden_act=hidden_act,
                       output_act=output_act)
    try:
        upload_dice_slabs(ctx, all_slabs)
        theta = t64.astype(np.float32)
        ctx.set_theta(theta)
        ctx.set_step_sizes(np.full(ctx.n_params, c['alpha'], np.float32))
        zeros = np.zeros(K, np.float32)
        # inner step
        ctx.switch_to_pre_update()
        ctx.inner_adapt(0, _lib.INNER_DICE)
        e_adapt = rel_max(ctx.get_task_thetas() - theta, ad - t64)
        # DICE-MAML: exact meta-gradient, and the same call without the coupling term
        grad, _ = ctx.meta_grad(0.0, zeros, _lib.INNER_DICE, _lib.OUTER_LOGLIK)
        e_dice = {name: rel_max(grad, g) for name, _, g in refs['dice']}
        grad_ll, _ = ctx.meta_grad(0.0, zeros, _lib.INNER_LOGLIK, _lib.OUTER_LOGLIK)
        e_ll = rel_max(grad_ll, refs['dice'][0][2])
        # VPG-DiCE-MAML: the last step's weights are the advantages
        ctx.set_advantages(K, np.concatenate([sl['vpg_advantages'] for sl in all_slabs[K]]).astype(np.float32))
        grad_v, st = ctx.meta_grad(0.0, zeros, _lib.INNER_DICE, _lib.OUTER_LOGLIK)
        e_vpg = {name: rel_max(grad_v, g) for name, _, g in refs['vpg']}
        e_cross = rel_max(grad, refs['vpg'][0][2])
        if verbose:
            print('dice-shape %s %s/%s: adapt %.2e  dice %s  loglik-only %.2e  vpg %s  dice-vs-vpg %.2e' % (
                {k: c[k] for k in ('M', 'P', 'T', 'O', 'A', 'hidden', 'K')}, hidden_act, output_act, e_adapt, {k: '%.2e' % v for k, v in e_dice.items()}, e_ll, {k: '%.2e' % v for k, v in e_vpg.items()}, e_cross))
        assert e_adapt < tol
        for name, e in e_dice.items():
            assert e < tol, ('dice', name, e)
        assert e_ll > 10 * tol              # without the coupling term the gradient is measurably different
        for name, loss, _ in refs['vpg']:
            np.testing.assert_allclose(st['loss'], loss, rtol=1e-4, atol=1e-6)
        for name, e in e_vpg.items():
            assert e < tol, ('vpg', name, e)
        assert e_cross > 10 * tol           # the DiCE outer objective gives a measurably different gradient
        return grad
    finally:
        ctx.close()

