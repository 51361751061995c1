"""developer tool: wall time per vectorised environment step of a collection, two ways --

  host    promp_policy_step from page-locked host arrays: upload the observations, launch, download the actions, synchronise
          (the only way before the promp_*_dev entry points);
  device  promp_policy_step_dev + promp_file_step_dev on device arrays: two launches and four event operations, no copy, no
          synchronisation per step (one at the end of the collection, counted).

The "environment" is a copy of precomputed observations into the array the policy reads: host to host in page-locked memory for the
first, device to device on a stream of the tool's own for the second -- an environment that costs next to nothing, so the figures
are the library's overhead per step, not a simulator's.  Shapes: the rollout shapes of config 1 (40 x 20 environments, obs 2,
act 2, (32, 32)) and of config 3 (40 x 20, obs 20, act 6, (64, 64)).  A loop is one collection of --steps vectorised steps; the
two ways alternate, --warmup loops each are dropped, the median of --loops loops each is reported with the fastest and slowest.
Also: one promp_collection_progress call (a launch, a 24-byte download, a synchronise) on a drained queue.

    python tools/device_env_timing.py [--steps 100] [--loops 21] [--warmup 3] [--out profiles/device_env_timing.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from promp_amd import _lib, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=100)
ap.add_argument('--loops', type=int, default=21)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'device_env_timing.txt'))
args = ap.parse_args()

SHAPES = (('config 1', 40, 20, 2, 2, (32, 32)), ('config 3', 40, 20, 20, 6, (64, 64)))
POOL = 8                       # precomputed observation sets the "environment" cycles through
SEED = 0x9E3779B97F4A7C15

lib = _lib.get_library()
hip = C.CDLL('libamdhip64.so')
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
hip.hipStreamSynchronize.argtypes = [C.c_void_p]
hip.hipStreamDestroy.argtypes = [C.c_void_p]
HIP_D2D, HIP_STREAM_NON_BLOCKING = 3, 1
lines = []


def say(text=''):
    print(text)
    lines.append(text)


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


for name, M, B, O, A, hidden in SHAPES:
    n, S = M * B, args.steps
    ctx = _lib.Context(M, O, A, hidden, 1, max_rows=S * n, max_paths=S * n, lib=lib)
    if name == SHAPES[0][0]:
        info = ctx.device_info()
        say('device: %s, %d CUs, %d MHz; %d steps per collection, median [fastest, slowest] of %d loops after %d warm-up loops'
            % (info['name'], info['n_cus'], info['clock_mhz'], S, args.loops, args.warmup))
        say('%-10s %-8s %28s %28s' % ('shapes', 'way', 'us per vectorised step', 'ms per collection'))
    rng = np.random.RandomState(1)
    ctx.set_theta(synthetic.init_theta(rng, O, hidden, A))
    ctx.switch_to_pre_update()
    pool_host = _lib.pinned_empty(lib, (POOL, n, O))
    pool_host[...] = rng.randn(POOL, n, O).astype(np.float32)
    obs_host, act_host = _lib.pinned_empty(lib, (n, O)), _lib.pinned_empty(lib, (n, A))
    pool_dev = ctx.device_array((POOL, n, O)).upload(pool_host)
    obs_dev, act_dev = ctx.device_array((n, O)), ctx.device_array((n, A))
    rew_dev = ctx.device_array((n,)).upload(rng.randn(n))
    done_dev, ended_dev = ctx.device_array((n,), np.uint8).upload(np.zeros(n)), ctx.device_array((n,), np.uint8)
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), HIP_STREAM_NON_BLOCKING) == 0
    obs_bytes = n * O * 4
    p_obs_host, p_act_host = obs_host.ctypes.data_as(C.POINTER(C.c_float)), act_host.ctypes.data_as(C.POINTER(C.c_float))

    def host_loop():
        ctx.begin_collection(0, B, S)
        t0 = time.perf_counter()
        for s in range(S):
            obs_host[...] = pool_host[s % POOL]
            ctx._call('promp_policy_step', 0, s, p_obs_host, SEED, 1, p_act_host)
        return time.perf_counter() - t0

    def device_loop():
        ctx.begin_collection(0, B, S)
        t0 = time.perf_counter()
        for s in range(S):
            hip.hipMemcpyAsync(obs_dev.ptr, pool_dev.ptr + (s % POOL) * obs_bytes, obs_bytes, HIP_D2D, stream)
            ctx._call('promp_policy_step_dev', 0, s, obs_dev.ptr, SEED, 1, act_dev.ptr, stream)
            ctx._call('promp_file_step_dev', 0, s, rew_dev.ptr, done_dev.ptr, S, ended_dev.ptr, stream)
        ctx.sync()
        hip.hipStreamSynchronize(stream)
        return time.perf_counter() - t0

    times = dict(host=[], device=[])
    for loop in range(args.warmup + args.loops):
        for way, fn in (('host', host_loop), ('device', device_loop)):
            t = fn()
            if loop >= args.warmup:
                times[way].append(t)
    for way in ('host', 'device'):
        m, lo, hi = med(times[way])
        say('%-10s %-8s %10.2f [%7.2f, %7.2f] %10.3f [%7.3f, %7.3f]'
            % (name, way, 1e6 * m / S, 1e6 * lo / S, 1e6 * hi / S, 1e3 * m, 1e3 * lo, 1e3 * hi))
    # the last device loop's collection is still open, every step filed, the queue drained
    prog = []
    for _ in range(args.warmup + args.loops):
        t0 = time.perf_counter()
        ctx.collection_progress(0, S * n)
        prog.append(time.perf_counter() - t0)
    m, lo, hi = med(prog[args.warmup:])
    say('%-10s %-8s %10.2f [%7.2f, %7.2f] us per promp_collection_progress call over %d filed steps' % (name, 'progress', 1e6 * m, 1e6 * lo, 1e6 * hi, S))
    for a in (pool_dev, obs_dev, act_dev, rew_dev, done_dev, ended_dev):
        a.free()
    hip.hipStreamDestroy(stream)
    ctx.close()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as f:
    f.write('\n'.join(lines) + '\n')
