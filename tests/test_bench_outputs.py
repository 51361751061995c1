"""bench.py's plain run and --dump-outputs, end to end on the kernel emulator (no GPU): a plain run times exactly --steps steps in
one loop and carries none of the --full measurements; --dump-outputs writes what the last timed step computed as float32 / float64
.npy files, and the same arguments give the same inputs, hence the same outputs."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ('roofline', 'h2d', 'plugin_path', 'cpu_baseline', 'exact_hvp', 'host_cg_loop', 'rccl', 'weak_batch', 'fixed_batch')


def _run(out_dir, *extra):
    from tests import devlib
    devlib.emu_library()
    env = dict(os.environ, PROMP_EMU_CUS='2', PYTHONPATH=ROOT)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, 'tests', 'bench_emu_driver.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
           '--test-shape', '4,2,12,5,3,32', '--dump-outputs', str(out_dir)] + list(extra)
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1500, cwd=ROOT)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.startswith('{')]
    assert len(lines) == 1, 'exactly one JSON line'
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith('.npy')}


def test_plain_run_times_its_steps_and_dumps_the_last_step(tmp_path):
    a, b = tmp_path / 'a', tmp_path / 'b'
    d = _run(a)
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in d
    assert d['steps'] == 3 and d['warmup'] == 1 and len(d['timed_loops_ms_per_step']) == 1
    assert d['ms_per_step'] > 0 and d['value'] > 0 and d['higher_is_better'] is True
    assert abs(d['value'] - d['config']['env_steps_per_step'] / (d['ms_per_step'] * 1e-3)) <= 1e-6 * d['value']
    assert not [k for k in FULL_ONLY if k in d], 'a plain run measures nothing beyond its timed steps'
    out = _load(a)
    M, R, n_params = 4, 4 * 2 * 12, 5 * 32 + 32 + 32 * 32 + 32 + 32 * 3 + 3 + 3
    assert out['theta'].shape == (n_params,) and out['adapted_task_params'].shape == (M, n_params)
    for k in (0, 1):
        assert out['advantages_step%d' % k].shape == (R,) and out['returns_step%d' % k].shape == (R,)
        assert out['baseline_coeffs_step%d' % k].shape[0] == M
    for k in ('loss_before', 'loss_after', 'inner_kl', 'outer_kl'):
        assert k in out
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) <= 64 << 20
    for name, v in out.items():
        assert v.dtype in (np.float32, np.float64), name
        assert np.all(np.isfinite(v)), name
    # the theta the outer step left differs from the seeded initial one: the dump is of the steps, not of the set-up
    assert np.abs(out['theta'] - out['adapted_task_params'][0]).max() > 0
    # the same arguments: the same seeded inputs, the same outputs
    _run(b)
    again = _load(b)
    assert sorted(again) == sorted(out)
    for name in out:
        np.testing.assert_allclose(again[name], out[name], rtol=1e-5, atol=1e-6, err_msg=name)
