"""Developer tool: what the outer optimiser's settings (promp_set_outer_optimizer) cost, and that a change costs nothing.
One promp_optimize of E = 5 epochs from resident slabs at BASELINE config 3's and config 4's shapes, in five variants: nothing
set, PROMP_OUTER_GENERIC=1 (default arguments on the general kernels), SGD, clipping on (Adam, a clip that is never active: the
launches are what counts), and trained step sizes.  With --parent-lib EVERY variant runs on a library built from the parent commit
too.  All contexts are interleaved round by round in one process so that they share whatever else the machine is doing.
A context's place in the process costs something of its own (the first context of a pair measured 3 to 4 us per call slower at
config 3 whichever library it bound, profiles/final_stage_dedup_timing.txt), so with --parent-lib every variant has two contexts
per library, created and timed in the order branch, parent, parent, branch, and a library's per-round mean is the mean of its two.
Per variant and library: the median over the rounds and the spread (min .. max) of the per-round means.  With --parent-lib the
tool exits with status 1 unless, for every variant, the branch's median lies inside the parent's own min .. max.
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
        def make(which, variant):
            if variant == 'PROMP_OUTER_GENERIC=1':
                os.environ['PROMP_OUTER_GENERIC'] = '1'          # (read when a context is created)
            ctx = make_ctx(which, M, P, T, O, A, hidden, variant == 'step sizes trained')
            os.environ.pop('PROMP_OUTER_GENERIC', None)
            if variant == 'sgd':
                ctx.set_outer_optimizer('sgd')
            if variant == 'clipping on':
                ctx.set_outer_optimizer('adam', None, max_grad_norm=1e30)
            return ctx
        names = ['nothing set', 'PROMP_OUTER_GENERIC=1', 'sgd', 'clipping on', 'step sizes trained']
        variants = []
        for v in names:
            order = [('branch, ' + v, lib)] if parent is None else [('branch, ' + v, lib), ('parent, ' + v, parent),
                                                                        ('parent, ' + v, parent), ('branch, ' + v, lib)]
            variants += [(n, make(which, v)) for n, which in order]
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
            took = {n: [] for n in ms}
            for n, ctx in variants:
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step(ctx)
                ctx.sync()
                took[n].append((time.perf_counter() - t0) / args.steps * 1e3)
            for n in ms:
                ms[n].append(float(np.mean(took[n])))
        say('%s   Theta %d' % (name, ctx0.n_params))
        for n in ms:
            v = np.array(ms[n])
            say('    %-36s median %8.3f ms   spread %8.3f .. %8.3f ms' % (n, np.median(v), v.min(), v.max()))
        base = float(np.median(ms['branch, nothing set']))
        for v in names[1:]:
            d = float(np.median(ms['branch, ' + v])) - base
            say('    %-36s %+8.3f ms per call = %+7.2f us per epoch against nothing set' % ('branch, ' + v, d, d / EPOCHS * 1e3))
        for v in names if parent is not None else ():
            b, p = float(np.median(ms['branch, ' + v])), np.array(ms['parent, ' + v])
            inside = p.min() <= b <= p.max()
            say('    requirement, %s: the branch\'s median (%.3f ms) inside the parent\'s min .. max (%.3f .. %.3f ms): %s'
                % (v, b, p.min(), p.max(), 'holds' if inside else 'DOES NOT HOLD'))
            ok = ok and inside
        for _, ctx in variants:
            ctx.close()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
