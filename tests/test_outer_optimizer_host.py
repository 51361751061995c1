"""The outer step's planning in promp_amd/csrc/promp_plan.h -- rule names, the validation of promp_set_outer_optimizer's arguments,
the constants default arguments give, which final-stage kernels run and on which grids -- on the host alone: tests/host/outer_opt_check.cpp
includes the plan header and nothing else of the project, is built with AddressSanitizer and UBSan, and says what does not hold.
The binding's own table of names must agree with the header's.  No GPU, no emulator."""
import os
import re
import shutil
import subprocess

from promp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host', 'outer_opt_check.cpp')


def test_outer_opt_check(tmp_path):
    gxx = shutil.which('g++')
    assert gxx, 'g++ is required'
    exe = str(tmp_path / 'outer_opt_check')
    r = subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-Wall', '-Wextra',
                        SRC, '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, 'outer_opt_check failed:\n' + r.stdout + r.stderr
    assert 'all expectations hold' in r.stdout


def test_binding_names_match_the_header():
    txt = open(os.path.join(ROOT, 'include', 'promp_hip.h')).read()
    enum = dict((k.lower(), int(v)) for k, v in re.findall(r'PROMP_OUTER_(ADAM|SGD|MOMENTUM) = (\d)', txt))
    assert enum == _lib.OUTER_RULES
    for name, rule in (('adam', 0), (None, 0), ('sgd', 1), ('gradient_descent', 1), ('momentum', 2)):
        assert _lib.outer_rule_id(name) == rule
    for cls, rule in (('AdamOptimizer', 0), ('GradientDescentOptimizer', 1), ('MomentumOptimizer', 2)):
        assert _lib.outer_rule_id(type(cls, (), {})) == rule
    args, lr = _lib.outer_rule_args(0, dict(epsilon=1e-5, learning_rate=3e-4))
    assert args.tolist() == [float(_lib.np.float32(x)) for x in (0.9, 0.999, 1e-5, 0.0)] and lr == 3e-4
    args, lr = _lib.outer_rule_args(2, dict(momentum=0.5, use_nesterov=True))
    assert args.tolist() == [0.5, 1.0, 0.0, 0.0] and lr is None
