"""Developer tool: what ProMP's num_minibatches costs.  BASELINE config 3's shapes (40 tasks x 20 paths x 200 rows, (64,64), obs 20,
act 6, K = 1), E = 5 epochs; the parameters and the Adam slots are put back before every call.  For B in {1, 2, 4}:
  draw     the E x (K + 1) assignments on the host (minibatch_assignment: one permutation per task, epoch and sampling step)
  begin    promp_optimize_minibatch_begin until it returns (validation, the tables of every epoch's slabs, all enqueues)
  call     begin + promp_optimize_end: one optimize_policy without the draw; and the same per Adam step (E x B of them)
  scatter  k_scatter_partition, HIP events around every launch in a run of their own (the events cost queue bubbles, so the
           other figures are taken with profiling off): microseconds per launch, and the bytes one launch reads plus writes
B = 1 is promp_optimize_begin itself; run against a tree that lacks the entry point (--parent) it times Context.optimize_begin /
optimize_end, the same call.  Per figure the median over the repetitions and the spread (min .. max).
usage: python tools/minibatch_timing.py [--reps N] [--parent]"""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from promp_amd import _lib, synthetic

M, P, T, O, A, HIDDEN, K = 40, 20, 200, 20, 6, (64, 64), 1
E, LR, CLIP = 5, 1e-3, 0.3


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
            ctx.inner_adapt(k)
            th = ctx.get_task_thetas()
    ctx.set_theta(theta0)
    return ctx, theta0


def stats(v):
    v = np.asarray(v)
    return 'median %8.3f   spread %8.3f .. %8.3f' % (np.median(v), v.min(), v.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--parent', action='store_true', help='B = 1 only, through optimize_begin / optimize_end')
    args = ap.parse_args()
    ctx, theta0 = make_ctx(_lib.get_library())
    eta = np.full(K, 5e-4, np.float32)
    zero = np.zeros(ctx.n_params, np.float32)
    print('measured %s on %s: %d repetitions per figure; %d tasks x %d paths x %d rows, %s, obs %d, act %d, K = %d, E = %d' %
          (time.strftime('%Y-%m-%d'), ctx.device_info(), args.reps, M, P, T, HIDDEN, O, A, K, E))
    if not args.parent:
        from promp_amd.optimizers.maml_first_order_optimizer import minibatch_assignment
    for B in ((1,) if args.parent else (1, 2, 4)):
        draw_ms, begin_ms, call_ms, scat = [], [], [], None
        np.random.seed(5)
        for rep in range(args.reps + 3):                # (two warm-up repetitions; the last one under the profiler)
            profiled = rep == args.reps + 2
            ctx.set_theta(theta0)
            ctx.set_adam_state(zero, zero, 0)
            if profiled:
                if B == 1:
                    break
                ctx.prof_enable(True)
                before = ctx.prof_read(_lib.KERNEL_SCATTER)
            ctx.sync()
            t0 = time.perf_counter()
            assign = None if B == 1 else [[minibatch_assignment([P] * M, B) for _ in range(K + 1)] for _ in range(E)]
            t1 = time.perf_counter()
            if args.parent:
                ctx.optimize_begin(E, LR, CLIP, eta)
            else:
                ctx.optimize_minibatch_begin(E, B, assign, LR, CLIP, eta)
            t2 = time.perf_counter()
            res = ctx.optimize_end()
            t3 = time.perf_counter()
            if profiled:
                after = ctx.prof_read(_lib.KERNEL_SCATTER)
                ctx.prof_enable(False)
                n = after['launches'] - before['launches']
                scat = (1e3 * (after['total_ms'] - before['total_ms']) / n, n, (after['rows'] - before['rows']) // n)
            elif rep >= 2:
                draw_ms.append((t1 - t0) * 1e3)
                begin_ms.append((t2 - t1) * 1e3)
                call_ms.append((t3 - t1) * 1e3)
        print('  B = %d   Adam steps %2d   loss %.6f -> %.6f' % (B, E * B, res['loss_before'], res['loss_after']))
        print('          draw ms           %s' % stats(draw_ms))
        print('          begin ms          %s' % stats(begin_ms))
        print('          call ms           %s' % stats(call_ms))
        print('          ms per Adam step  %s' % stats(np.asarray(call_ms) / (E * B)), flush=True)
        if scat:
            # per row: observations, the advantage, actions and old means (log_std is one row per task here), read and written
            nbytes = 2 * 4 * scat[2] * (O + 1 + 2 * A)
            print('          scatter: %d launches, %.1f us each, %d rows and %.2f MB read + written per launch (%.0f GB/s)' %
                  (scat[1], scat[0], scat[2], nbytes / 1e6, nbytes / scat[0] / 1e3), flush=True)
    ctx.close()


if __name__ == '__main__':
    main()
