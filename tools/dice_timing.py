"""Developer tool: one DICE-MAML outer step (promp_optimize: 1 epoch, PROMP_INNER_DICE / PROMP_OUTER_LOGLIK, K = 1) from resident
slabs, one shape per pass-kernel family, beside the PROMP_INNER_LOGLIK step on the same slabs.  The DiCE step is the
log-likelihood step plus, per inner step, one k_dice_scan and one first-order pass (the coupling term).
usage: python tools/dice_timing.py [--steps N] [--case I]"""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from promp_amd import _lib, synthetic

CASES = [   # name, M, P, T, O, A, hidden
    ('Chain      config 3: (64,64), obs 20, act 6', 40, 20, 200, 20, 6, (64, 64)),
    ('CoopSplit  config 4: (128,128), obs 111, act 8', 40, 20, 200, 111, 8, (128, 128)),
    ('CoopFp32   (64,64), obs 111, act 8', 40, 20, 200, 111, 8, (64, 64)),
    ('Layered    Humanoid: (64,64), obs 376, act 17', 40, 20, 200, 376, 17, (64, 64)),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--case', type=int, default=-1, help='run only this entry of CASES')
    args = ap.parse_args()
    HEAD = '%-50s %7s %10s %10s %8s   %s' % ('shape', 'Theta', 'DiCE ms', 'loglik ms', 'ratio', 'passes per step: DiCE | loglik (fwd+bwd, R-op)')
    first = True
    for name, M, P, T, O, A, hidden in (CASES if args.case < 0 else CASES[args.case:args.case + 1]):
        K, N = 1, P * T
        rng = np.random.RandomState(3)
        theta0 = synthetic.init_theta(np.random.RandomState(1), O, hidden, A)
        ctx = _lib.Context(M, O, A, hidden, K, max_rows=M * N, max_paths=M * P)
        if first:
            print('measured %s on %s, %d steps per figure' % (time.strftime('%Y-%m-%d'), ctx.device_info(), args.steps))
            print(HEAD)
            first = False
        ctx.set_theta(theta0)
        ctx.set_step_sizes(np.full(ctx.n_params, 0.1, np.float32))
        ids = list(range(M))
        th = theta0
        for k in range(K + 1):
            f = _lib.flatten_paths(synthetic.make_paths_for_tasks(7 + k, ids, th, P, T, O, A, hidden))
            ls = np.tile(theta0[-A:], (M, 1)) if k == 0 else th[:, -A:].copy()
            ctx.upload_step(k, f['task_path_offsets'], f['path_row_offsets'], f['obs'], f['rew'], f['act'], f['old_mean'], ls)
            # adjusted rewards ~ N(0, 1), scaled as the DiCE sample processor does (rows / (paths * max_path_length) = 1 here)
            ctx.set_dice_rewards(k, rng.randn(M * N).astype(np.float32))
            if k < K:
                ctx.switch_to_pre_update()
                ctx.inner_adapt(k, _lib.INNER_DICE)
                th = ctx.get_task_thetas()
        ctx.set_theta(theta0)      # (new parameter version: neither kind of step finds the inner pass promp_inner_adapt left behind)
        eta = np.zeros(K, np.float32)

        def timed(inner_kind):
            # lr = 0: the parameters (and with them the work) stay the same from step to step
            step = lambda: ctx.optimize(1, 0.0, 0.0, eta, inner_kind, _lib.OUTER_LOGLIK)
            for _ in range(3):
                step()
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            ctx.sync()
            ms = (time.perf_counter() - t0) / args.steps * 1e3
            ctx.prof_enable(True)
            step()
            ctx.sync()
            prof = [ctx.prof_read(kid) for kid in (0, 1)]
            ctx.prof_enable(False)
            return ms, '%d x %.0f us, %d x %.0f us' % tuple(x for v in prof for x in (v['launches'], 1e3 * v['total_ms'] / max(v['launches'], 1)))
        d_ms, d_prof = timed(_lib.INNER_DICE)
        l_ms, l_prof = timed(_lib.INNER_LOGLIK)
        print('%-50s %7d %10.3f %10.3f %8.2f   %s | %s' % (name, ctx.n_params, d_ms, l_ms, d_ms / l_ms, d_prof, l_prof), flush=True)
        ctx.close()


if __name__ == '__main__':
    main()
