"""Developer tool: what the outer optimiser's settings (promp_set_outer_optimizer) cost, and that the default path costs nothing.
One promp_optimize of E = 5 epochs from resident slabs at BASELINE config 3's and config 4's shapes: the branch with nothing set,
with --parent-lib the same call of a library built from the parent commit, then the branch with PROMP_OUTER_GENERIC=1 (default
arguments on the general kernels), under SGD, and with clipping on (Adam, a clip that is never active: the launches are what
counts).  The variants are interleaved round by round in one process so that they share whatever else the machine is doing.
Per variant: the median over the rounds and the spread (min .. max) of the per-round means.  With --parent-lib the tool exits
with status 1 unless the median of `branch, nothing set` lies inside the parent's own min .. max.
From the launch schedule: the general kernels add no launch; the clip replaces the fused final launch by two dependent ones.
usage: python tools/outer_optimizer_timing.py [--steps N] [--rounds R] [--parent-lib PATH] [--out FILE]"""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from promp_amd import _lib
from tools.step_size_timing import CASES, EPOCHS, OlderLibrary, make_ctx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20, help='promp_optimize calls per round and variant')
    ap.add_argument('--rounds', type=int, default=8)
    ap.add_argument('--parent-lib', default=None, help='libpromp_hip.so built from the parent commit')
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    lib = _lib.get_library()
    parent = OlderLibrary(args.parent_lib) if args.parent_lib else None
    eta = np.array([5e-4], np.float32)
    ok = True
    for ci, (name, M, P, T, O, A, hidden) in enumerate(CASES):
        variants = [('branch, nothing set', make_ctx(lib, M, P, T, O, A, hidden, False))]
        if parent is not None:
            variants.append(('parent', make_ctx(parent, M, P, T, O, A, hidden, False)))
        os.environ['PROMP_OUTER_GENERIC'] = '1'              # (read when a context is created)
        variants.append(('branch, PROMP_OUTER_GENERIC=1', make_ctx(lib, M, P, T, O, A, hidden, False)))
        del os.environ['PROMP_OUTER_GENERIC']
        sgd = make_ctx(lib, M, P, T, O, A, hidden, False)
        sgd.set_outer_optimizer('sgd')
        variants.append(('branch, sgd', sgd))
        clip = make_ctx(lib, M, P, T, O, A, hidden, False)
        clip.set_outer_optimizer('adam', None, max_grad_norm=1e30)
        variants.append(('branch, clipping on', clip))
        ctx0 = variants[0][1]
        if ci == 0:
            say('measured %s on %s: %d rounds x %d calls of promp_optimize(E = %d) per variant, interleaved' %
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
        say('%s   Theta %d' % (name, ctx0.n_params))
        for n, _ in variants:
            v = np.array(ms[n])
            say('    %-30s median %8.3f ms   spread %8.3f .. %8.3f ms' % (n, np.median(v), v.min(), v.max()))
        base = float(np.median(ms['branch, nothing set']))
        for n in ('branch, PROMP_OUTER_GENERIC=1', 'branch, sgd', 'branch, clipping on'):
            d = float(np.median(ms[n])) - base
            say('    %-30s %+8.3f ms per call = %+7.2f us per epoch against nothing set' % (n, d, d / EPOCHS * 1e3))
        if parent is not None:
            p = np.array(ms['parent'])
            inside = p.min() <= base <= p.max()
            say('    requirement: median of `branch, nothing set` (%.3f ms) inside the parent\'s min .. max (%.3f .. %.3f ms): %s'
                % (base, p.min(), p.max(), 'holds' if inside else 'DOES NOT HOLD'))
            ok = ok and inside
        for _, ctx in variants:
            ctx.close()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
