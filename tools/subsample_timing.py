"""Developer tool: what ConjugateGradientOptimizer's subsample_factor buys.  BASELINE config 5's shapes (TRPO-MAML on config 3's:
40 tasks x 20 paths x 200 rows, (64,64), obs 20, act 6, K = 1) with an on-policy batch (the last step's old distribution is
the adapted policy's own, so steps are accepted); the parameters are put back before every step.  For hvp_mode 0 (the
reference's symmetric finite differences) and 2 (the exact product), at f in {1, 0.5, 0.2, 0.1}:
  select  drawing the subsample on the host (one np.random.choice per task and sampling step) and setting it
  solve   select, promp_cg_solve (10 iterations + the closing product; the first product copies the selected rows), clearing
  step    ConjugateGradientOptimizer.optimize(): loss gradient, select, the solve, the line search (one forward evaluation per
          candidate: how many it tries depends on the direction, so it is printed)
  cosine  between the direction at f < 1 (one draw per repetition) and the direction at f = 1 on the same batch
Per figure the median over the repetitions and the spread (min .. max).
usage: python tools/subsample_timing.py [--reps N]"""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from promp_amd import _lib, synthetic
from promp_amd.meta_algos.trpo_maml import _DeviceEvaluator
from promp_amd.optimizers.conjugate_gradient_optimizer import ConjugateGradientOptimizer, ExactDeviceHvp, FiniteDifferenceHvp
from promp_amd.utils import logger

M, P, T, O, A, HIDDEN, K = 40, 20, 200, 20, 6, (64, 64), 1
FACTORS = (1., 0.5, 0.2, 0.1)


class OneContext(object):
    """what TRPOMAML's evaluator asks of its algorithm and session, over one resident context"""
    exploration, inner_kind, num_inner_grad_steps, M_global = False, _lib.INNER_LOGLIK, K, M

    def __init__(self, ctx):
        self.ctx, self.session = ctx, self

    def external(self):
        return False

    def meta_eval(self, clip_eps, eta, inner_kind, outer_kind):
        return self.ctx.meta_grad(clip_eps, eta, inner_kind=inner_kind, outer_kind=outer_kind)[1]


def make_ctx(lib):
    theta0 = synthetic.init_theta(np.random.RandomState(1), O, HIDDEN, A)
    ctx = _lib.Context(M, O, A, HIDDEN, K, max_rows=M * P * T, max_paths=M * P, lib=lib)
    ctx.set_theta(theta0)
    ctx.set_step_sizes(np.full(ctx.n_params, 0.1, np.float32))
    th = theta0
    for k in range(K + 1):
        f = _lib.flatten_paths(synthetic.make_paths_for_tasks(7 + k, list(range(M)), th, P, T, O, A, HIDDEN))
        ls = np.tile(theta0[-A:], (M, 1)) if k == 0 else th[:, -A:].copy()
        ctx.upload_step(k, f['task_path_offsets'], f['path_row_offsets'], f['obs'], f['rew'], f['act'], f['old_mean'], ls)
        ctx.process_samples(k, baseline_kind=1, discount=0.99, gae_lambda=1.0, normalize_adv=True)
        if k < K:
            ctx.switch_to_pre_update()
            ctx.inner_adapt(k, inner_kind=_lib.INNER_LOGLIK)
            th = ctx.get_task_thetas()
    ctx.set_theta(theta0)
    return ctx, theta0


def stats(v):
    v = np.asarray(v)
    return 'median %8.3f   spread %8.3f .. %8.3f' % (np.median(v), v.min(), v.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    args = ap.parse_args()
    logger.configure(dir=None, quiet=True)
    ctx, theta0 = make_ctx(_lib.get_library())
    algo = OneContext(ctx)
    ev = _DeviceEvaluator(algo)
    print('measured %s on %s: %d repetitions per figure; %d tasks x %d paths x %d rows, %s, obs %d, act %d, K = %d' %
          (time.strftime('%Y-%m-%d'), ctx.device_info(), args.reps, M, P, T, HIDDEN, O, A, K))
    eta = np.zeros(K, np.float32)
    b = ctx.meta_grad(0.0, eta, inner_kind=_lib.INNER_LOGLIK, outer_kind=_lib.OUTER_RATIO)[0]
    for mode, name in ((0, 'hvp_mode 0: symmetric finite differences'), (2, 'hvp_mode 2: exact product')):
        print(name)
        full = None
        for f in FACTORS:
            opt = ConjugateGradientOptimizer(subsample_factor=f, hvp_approach=ExactDeviceHvp() if mode == 2 else FiniteDifferenceHvp())
            opt.build_graph(ev, 0.01)
            select_ms, solve_ms, step_ms, cos, tried, accepted, kept = [], [], [], [], [], 0, None
            np.random.seed(5)
            for rep in range(args.reps + 2):            # (two warm-up repetitions)
                ctx.set_theta(theta0)
                ctx.sync()
                t0 = time.perf_counter()
                kept = ev.select_paths(f) if f < 1 else None
                ts = time.perf_counter()
                x, q = ctx.cg_solve(b, cg_iters=10, hvp_mode=mode, inner_kind=_lib.INNER_LOGLIK)
                ev.clear_selection()
                t1 = time.perf_counter()
                opt.optimize()
                ctx.sync()
                t2 = time.perf_counter()
                if f == 1. and full is None:
                    full = x.astype(np.float64)
                if rep >= 2:
                    select_ms.append((ts - t0) * 1e3)
                    solve_ms.append((t1 - t0) * 1e3)
                    step_ms.append((t2 - t1) * 1e3)
                    accepted += 0 if opt.last['rejected'] else 1
                    tried.append(opt.last['n_backtracks'] + 1)
                    d = opt.last['descent_direction'].astype(np.float64)
                    cos.append(float(d.dot(full) / (np.linalg.norm(d) * np.linalg.norm(full))))
            print('  f = %-4g paths per task %3d   select ms %s\n%s solve ms %s\n%s step ms %s\n%s cosine to f = 1: %s   accepted %d / %d' %
                  (f, kept[0][0] if kept else P, stats(select_ms), ' ' * 30, stats(solve_ms), ' ' * 31, stats(step_ms), ' ' * 21,
                   stats(cos), accepted, args.reps), flush=True)
            print('%s line-search candidates per step: %s' % (' ' * 21, ' '.join(str(t) for t in tried)), flush=True)
    ctx.set_theta(theta0)
    ctx.close()


if __name__ == '__main__':
    main()
