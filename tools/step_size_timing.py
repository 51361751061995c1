"""Developer tool: what trainable inner step sizes (promp_set_train_step_sizes) cost.  One promp_optimize of E = 5 epochs from
resident slabs at BASELINE config 3's and config 4's shapes, flag off and on; with --parent-lib also the flag-off call of a
library built from the parent commit, the three interleaved round by round in one process so that they share whatever else
the machine is doing.  Per variant: the median over the rounds and the spread (min .. max) of the per-round means.
From the launch schedule the flag adds one elementwise launch per inner step per epoch and Theta columns to the final stage.
usage: python tools/step_size_timing.py [--steps N] [--rounds R] [--parent-lib PATH]"""
import argparse, ctypes, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from promp_amd import _lib, synthetic

CASES = [   # name, M, P, T, O, A, hidden
    ('config 3: (64,64), obs 20, act 6', 40, 20, 200, 20, 6, (64, 64)),
    ('config 4: (128,128), obs 111, act 8', 40, 20, 200, 111, 8, (128, 128)),
]
EPOCHS = 5


class OlderLibrary(_lib.Library):
    """a library that may lack the newest entry points (the parent commit's): binds what it exports"""

    def __init__(self, path):
        self.path = path
        self.cdll = ctypes.CDLL(path)
        for name, (res, args) in _lib.SIGNATURES.items():
            fn = getattr(self.cdll, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = res, args


def make_ctx(lib, M, P, T, O, A, hidden, train):
    K, N = 1, P * T
    theta0 = synthetic.init_theta(np.random.RandomState(1), O, hidden, A)
    ctx = _lib.Context(M, O, A, hidden, K, max_rows=M * N, max_paths=M * P, lib=lib)
    ctx.set_theta(theta0)
    ctx.set_step_sizes(np.full(ctx.n_params, 0.1, np.float32))
    if train:
        ctx.set_train_step_sizes(True)
    th = theta0
    for k in range(K + 1):
        f = _lib.flatten_paths(synthetic.make_paths_for_tasks(7 + k, list(range(M)), th, P, T, O, A, hidden))
        ls = np.tile(theta0[-A:], (M, 1)) if k == 0 else th[:, -A:].copy()
        ctx.upload_step(k, f['task_path_offsets'], f['path_row_offsets'], f['obs'], f['rew'], f['act'], f['old_mean'], ls)
        ctx.process_samples(k, baseline_kind=1, discount=0.99, gae_lambda=1.0, normalize_adv=True)
        if k < K:
            ctx.switch_to_pre_update()
            ctx.inner_adapt(k)
            th = ctx.get_task_thetas()
    ctx.set_theta(theta0)
    return ctx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20, help='promp_optimize calls per round and variant')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--parent-lib', default=None, help='libpromp_hip.so built from the parent commit')
    args = ap.parse_args()
    lib = _lib.get_library()
    parent = OlderLibrary(args.parent_lib) if args.parent_lib else None
    eta = np.array([5e-4], np.float32)
    for ci, (name, M, P, T, O, A, hidden) in enumerate(CASES):
        variants = [('branch, flag off', make_ctx(lib, M, P, T, O, A, hidden, False))]
        if parent is not None:
            variants.append(('parent, (no flag)', make_ctx(parent, M, P, T, O, A, hidden, False)))
        variants.append(('branch, flag on', make_ctx(lib, M, P, T, O, A, hidden, True)))
        ctx0 = variants[0][1]
        if ci == 0:
            print('measured %s on %s: %d rounds x %d calls of promp_optimize(E = %d) per variant, interleaved' %
                  (time.strftime('%Y-%m-%d'), ctx0.device_info(), args.rounds, args.steps, EPOCHS))
        # lr = 0: the parameters (and with them the work) stay the same from call to call
        step = lambda ctx: ctx.optimize(EPOCHS, 0.0, 0.3, eta)
        for _, ctx in variants:
            for _ in range(3):
                step(ctx)
            ctx.sync()
        ms = {n: [] for n, _ in variants}
        for _ in range(args.rounds):
            for n, ctx in variants:
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step(ctx)
                ctx.sync()
                ms[n].append((time.perf_counter() - t0) / args.steps * 1e3)
        n_par = ctx0.n_params
        print('%s   Theta %d, extra device memory with the flag on: (K+1) M Theta floats = %.2f MB' %
              (name, n_par, 2 * M * n_par * 4 / 1e6))
        for n, _ in variants:
            v = np.array(ms[n])
            print('    %-20s median %8.3f ms   spread %8.3f .. %8.3f ms' % (n, np.median(v), v.min(), v.max()), flush=True)
        for _, ctx in variants:
            ctx.close()


if __name__ == '__main__':
    main()
