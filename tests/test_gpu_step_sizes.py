"""Learned per-parameter inner step sizes (trainable_inner_step_size) on the MI355X: every pass-kernel family's inner step keeps
its gradient, the backward sweep multiplies it with the complete multiplier, the final stage sums, exchanges and Adam-steps the
Theta extra columns (tests/step_size_checks.py).  The shapes are the smallest at which each path can go wrong; every case asserts
rel_max < 1e-4 against the float64 references and bitwise equality wherever two device paths must agree."""
import os

import pytest

from promp_amd import _lib, session
from tests import devlib, dice_shape_checks as ds, step_size_checks as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    return devlib.gpu_library()


@pytest.fixture(scope='module')
def shape1():                 # chain kernels, K 1
    return sc.PrompCase(601, M=3, P=2, T=50, O=7, A=3, hidden=(32, 32), K=1, ragged=True)


@pytest.fixture(scope='module')
def shape2():                 # chain kernels, lam carried through two steps
    return sc.PrompCase(602, M=3, P=2, T=50, O=20, A=6, hidden=(64, 64), K=2, ragged=True)


@pytest.fixture
def product_library():
    _lib.set_library_for_testing(None)      # the plugin classes bind promp_amd/libpromp_hip.so
    yield
    session._current = None


def test_references_agree(shape1, shape2):
    sc.check_references(shape1)
    sc.check_references(shape2)


def test_chain_kernels(lib, shape1):
    sc.check_alpha_grad(lib, shape1)


def test_chain_kernels_two_inner_steps(lib, shape2):
    sc.check_alpha_grad(lib, shape2)


def test_cooperative_split_kernels(lib):
    sc.check_alpha_grad(lib, sc.PrompCase(603, M=2, P=2, T=50, O=111, A=8, hidden=(128, 128), K=1))


def test_layer_by_layer_kernels(lib):
    sc.check_alpha_grad(lib, sc.PrompCase(604, M=3, P=2, T=50, O=20, A=6, hidden=(64, 64, 64), K=2))


def test_zero_padded_widths(lib):
    # (48, 20) runs on the (64, 32) kernels: alpha and its gradient cross the ABI in the caller's layout
    sc.check_alpha_grad(lib, sc.PrompCase(605, M=3, P=2, T=50, O=20, A=6, hidden=(48, 20), K=1))


def test_dice_inner_objective(lib):
    sc.check_dice_alpha_grad(lib, ds.case(606, M=2, P=2, T=40, O=7, A=3, hidden=(32, 32), K=2, ragged=True))


def test_learn_std_false(lib, shape1):
    sc.check_learn_std_false(lib, shape1, epochs=2)


def test_adam_on_step_sizes(lib, shape1):
    sc.check_adam(lib, shape1, epochs=3)


def test_split_path_equals_fused(lib):
    sc.check_split_equals_fused(lib, sc.PrompCase(609, M=5, P=2, T=50, O=7, A=3, hidden=(32, 32), K=1, ragged=True), epochs=2)


def test_reuse_adapt(lib, shape1):
    sc.check_reuse_adapt(lib, shape1)


def test_fused_and_separate_task_reduction_agree(lib, shape2):
    sc.check_schedule_invariance(lib, shape2)


def test_promp_plugin_trains_logs_and_snapshots_step_sizes(product_library, tmp_path):
    d = str(tmp_path / 'snap')
    trainer = sc.check_plugin('promp', 3, tmp_dir=d)
    sc.check_snapshot_round_trip(trainer, os.path.join(d, 'params.pkl'))


@pytest.mark.parametrize('algo', ['vpg', 'dice'])
def test_other_plugins_train_step_sizes(product_library, algo):
    sc.check_plugin(algo, 1)


def test_trpo_maml_keeps_step_sizes_constant(product_library):
    from promp_amd.meta_algos.trpo_maml import TRPOMAML
    from promp_amd.policies.meta_gaussian_mlp_policy import MetaGaussianMLPPolicy
    policy = MetaGaussianMLPPolicy(name='p', obs_dim=2, action_dim=2, meta_batch_size=2, hidden_sizes=(32, 32))
    algo = TRPOMAML(policy=policy, inner_lr=0.1, meta_batch_size=2, num_inner_grad_steps=1, trainable_inner_step_size=True)
    assert not algo.session.train_step_sizes


def test_optimizer_memo_covers_the_step_sizes(product_library):
    sc.check_memo_key()


def test_host_exchange_route_equals_optimize(lib, shape1):
    sc.check_host_exchange_route(lib, shape1)
