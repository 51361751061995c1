"""developer tool: one DiceMetaSampleProcessor.process_samples at config 3's shapes (40 tasks x 20 paths x 200 steps, obs 20, act 6,
LinearFeatureBaseline), with and without a LinearFeatureBaseline return baseline, from a batch resident on the device and from
host path dicts.  Each figure is split into the time spent inside the library's calls (uploads, launches, the blocking
downloads: "device") and the rest (Python and NumPy on the host: "host").

    python tools/dice_processing_timing.py [--reps N]
"""
import argparse
import os
import sys
import time
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from promp_amd import _lib, synthetic  # noqa: E402
from promp_amd.baselines.linear_baseline import LinearFeatureBaseline  # noqa: E402
from promp_amd.policies.meta_gaussian_mlp_policy import MetaGaussianMLPPolicy  # noqa: E402
from promp_amd.samplers.device_point_sampler import DevicePaths  # noqa: E402
from promp_amd.samplers.dice_sample_processor import DiceMetaSampleProcessor  # noqa: E402
from promp_amd.utils import logger as plog  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=10)
args = ap.parse_args()
plog.configure(quiet=True)
cfg = synthetic.CONFIGS[3]
M, P, T, O, A, hidden = cfg['M'], cfg['P'], cfg['T'], cfg['O'], cfg['A'], cfg['hidden']
theta0 = synthetic.init_theta(np.random.RandomState(3000), O, hidden, A)
policy = MetaGaussianMLPPolicy(name='p', obs_dim=O, action_dim=A, meta_batch_size=M, hidden_sizes=hidden, rank=0, world=1, device_id=0)
policy.set_params(policy._unflatten(theta0))
paths = synthetic.make_paths(np.random.RandomState(4321), theta0, M, P, T, O, A, hidden)
sess = policy.session

in_lib = [0.0]
_call = _lib.Context._call


def timed_call(self, name, *a):
    t0 = time.perf_counter()
    try:
        return _call(self, name, *a)
    finally:
        in_lib[0] += time.perf_counter() - t0


_lib.Context._call = timed_call


def resident_batch():
    fl = _lib.flatten_paths(paths)
    sess.upload_flat(0, fl)
    dp = DevicePaths(paths)
    dp.device_ref, dp.flat = (sess.serial, sess.upload_serial[0], 0), fl
    return dp


def host_batch():
    return OrderedDict((i, [dict(p, agent_infos=dict(p['agent_infos'])) for p in pl]) for i, pl in paths.items())


print('%-34s %10s %10s %10s   (ms per process_samples, %d x %d x %d, obs %d)' % ('', 'total', 'device', 'host', M, P, T, O))
for rb in (False, True):
    extra = dict(return_baseline=LinearFeatureBaseline()) if rb else {}
    proc = DiceMetaSampleProcessor(LinearFeatureBaseline(), max_path_length=T, discount=0.99, gae_lambda=1.0, normalize_adv=True, **extra)
    for name, make in (('resident batch', resident_batch), ('host path dicts', host_batch)):
        batch = make()
        for _ in range(3):
            proc.process_samples(batch, log=False)
        sess.ctx.sync()
        in_lib[0] = 0.0
        t0 = time.perf_counter()
        for _ in range(args.reps):
            proc.process_samples(batch, log=False)
            sess.ctx.sync()
        total = 1e3 * (time.perf_counter() - t0) / args.reps
        dev = 1e3 * in_lib[0] / args.reps
        print('%-34s %10.3f %10.3f %10.3f' % ('%s%s' % (name, ', return baseline' if rb else ''), total, dev, total - dev))
