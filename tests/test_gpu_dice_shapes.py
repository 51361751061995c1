"""DICE-MAML / VPG-DiCE-MAML on every pass-kernel family, on the MI355X: the cooperative FP32 kernels (k_wide_*), the
cooperative split kernels (k_wb_*), zero-padded widths embedded in them, and the layer-by-layer kernels (k_gen_* / k_gb_*),
through the C ABI (tests/dice_shape_checks.py: what parity_checks.check_dice and check_vpg_dice run) and through the plugin
classes (DiceMetaSampleProcessor -> DICEMAML._adapt -> optimize_policy).

Every case asserts rel_max < 1e-4 against the float64 references: oracle.dice and torch.autograd for tanh policies, the
torch.autograd transcription of dice_shape_checks.torch_dice_general (pinned against oracle.dice below) for the others."""
from collections import OrderedDict

import numpy as np
import pytest

from promp_amd import _lib, session
from tests import devlib, dice_shape_checks as ds

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    return devlib.gpu_library()


# The cooperative kernels walk a work item in rounds of 64 rows (32 in the R-operator pass), the layer-by-layer ones in blocks of
# 64 / 256 -- but a work item is what build_step_tables deals: one workgroup per compute unit, capped at one per 16-row tile.  On the
# 256 compute units of an MI355X every item of these small batches is ONE tile of at most 16 rows, so no case here takes a second
# round on hardware (the row counts noted below are those of a task, not of an item); tests/fused_checks.py and
# tests/layered_checks.py plan for one compute unit and do.
# `trim` entries (step, task, path, length) cut paths short: a path of ONE row, row counts that leave a partial last tile.
CASES = OrderedDict([
    # ---- CoopFp32: (64,64) with obs_dim > 32
    ('coopfp32_64_obs40', ds.case(401, M=3, P=3, T=50, O=40, A=3, hidden=(64, 64), ragged=True, trim=[(0, 1, 2, 1)])),
    ('coopfp32_64_obs111', ds.case(402, M=3, P=4, T=45, O=111, A=8, hidden=(64, 64))),                     # 180 rows a task: eleven tiles + 4 rows
    # ---- CoopSplit: (128,128), one per observation class (obs_dim <= 63 / <= 111 / <= 127)
    ('coopsplit_obs20', ds.case(403, M=3, P=3, T=60, O=20, A=6, hidden=(128, 128), ragged=True)),
    ('coopsplit_obs111', ds.case(404, M=3, P=4, T=45, O=111, A=8, hidden=(128, 128), trim=[(0, 0, 3, 1), (1, 2, 0, 7)])),
    ('coopsplit_obs127', ds.case(405, M=2, P=3, T=70, O=127, A=8, hidden=(128, 128), ragged=True)),
    # ---- zero-padded widths: (100,100) runs in (128,128), (48,20) at obs 40 in (64,64)
    ('padded_100_100', ds.case(406, M=3, P=3, T=50, O=50, A=4, hidden=(100, 100), ragged=True)),
    ('padded_48_20', ds.case(407, M=2, P=4, T=37, O=40, A=3, hidden=(48, 20))),                             # 148 rows a task: nine tiles + 4 rows
    # ---- Layered
    ('layered_64x3_k2', ds.case(408, M=2, P=3, T=40, O=20, A=6, hidden=(64, 64, 64), K=2, alpha=0.05, ragged=True)),
    ('layered_256_256', ds.case(409, M=2, P=3, T=90, O=20, A=6, hidden=(256, 256), trim=[(0, 0, 0, 1)])),  # task 0: 181 rows
    ('layered_humanoid', ds.case(410, M=2, P=3, T=50, O=376, A=17, hidden=(64, 64), ragged=True)),
    ('layered_100', ds.case(411, M=3, P=3, T=50, O=11, A=3, hidden=(100,))),
])
# 4 tasks x 20 paths x 200 steps at config-4 shapes (16 000 rows: many work items per task, nothing may depend on where the work
# items or their rounds end).  The float64 oracle and the two torch graphs take well under a minute at this size.
MID = ds.case(420, M=4, P=20, T=200, O=111, A=8, hidden=(128, 128), ragged=True)


def test_cases_cover_ragged_paths_partial_rounds_and_one_row_paths():
    ragged = [n for n, c in CASES.items() if c['ragged'] or c['trim']]
    assert 2 * len(ragged) >= len(CASES)
    partial, one_row = [], []
    for n, c in CASES.items():
        _, _, slabs = ds.make_case(c)
        if any(r % 32 for k in range(c['K']) for r in ds.task_rows(slabs, k)):
            partial.append(n)
        if any((ds.path_lengths(slabs, k) == 1).any() for k in range(c['K'])):
            one_row.append(n)
    assert {'coopfp32_64_obs111', 'padded_48_20', 'layered_256_256', 'coopsplit_obs111'} <= set(partial)
    assert {'coopfp32_64_obs40', 'coopsplit_obs111', 'layered_256_256'} <= set(one_row)


def test_general_torch_reference_is_the_oracle_on_tanh():
    ds.check_general_reference_against_oracle(ds.case(430, M=2, P=3, T=30, O=20, A=6, hidden=(64, 64, 64), K=2, alpha=0.05, ragged=True))
    ds.check_general_reference_against_oracle(ds.case(431, M=2, P=2, T=20, O=376, A=17, hidden=(64, 64), ragged=True))


@pytest.mark.parametrize('name', list(CASES))
def test_dice_and_vpg_dice_gradients(lib, name):
    ds.check_dice_shape(lib, CASES[name])


def test_dice_mid_size_config4_shapes(lib):
    ds.check_dice_shape(lib, MID)


# The kernel switches below are read with getenv() when a context is created, so they are set in this process around the one
# context the case creates (monkeypatch restores them); a child process started from the test process, which holds the device, was
# refused one on the MI355X box ("no HIP device available").  The switched kernels round differently from the default ones (FP32
# products against the two-term FP16 split, FP32 GEMMs against the BF16 pipe), so both runs meet the tolerance but never with the
# same bits: a gradient bitwise equal to the default path's would mean the switch was ignored and the case repeated the default.
def run_switched(lib, monkeypatch, name, switch):
    g_default = ds.check_dice_shape(lib, CASES[name])
    monkeypatch.setenv(switch, '1')
    g_switched = ds.check_dice_shape(lib, CASES[name])
    assert g_switched.shape == g_default.shape and not np.array_equal(g_switched, g_default)


def test_dice_coop_fp32_at_128_wide(lib, monkeypatch):
    # PROMP_WIDE_FP32=1: (128,128) at obs 111 on k_wide_* <128, 8> instead of k_wb_*
    run_switched(lib, monkeypatch, 'coopsplit_obs111', 'PROMP_WIDE_FP32')


def test_dice_layered_fp32_gemms(lib, monkeypatch):
    # PROMP_GEN_FP32=1: k_gen_linear / k_gen_wgrad in front of k_gen_loss instead of the BF16-pipe k_gb_*
    run_switched(lib, monkeypatch, 'layered_64x3_k2', 'PROMP_GEN_FP32')


@pytest.mark.parametrize('hidden_act,output_act,name', [('relu', None, 'relu_64x3'), ('tanh', 'tanh', 'tanh_out_humanoid')])
def test_dice_other_activations(lib, hidden_act, output_act, name):
    c = dict(relu_64x3=ds.case(440, M=2, P=3, T=40, O=20, A=6, hidden=(64, 64, 64), ragged=True),
             tanh_out_humanoid=ds.case(441, M=2, P=3, T=50, O=376, A=17, hidden=(64, 64), ragged=True))[name]
    ds.check_dice_shape(lib, c, hidden_act=hidden_act, output_act=output_act)


# ---- plugin level ------------------------------------------------------------------------------------------------------------

@pytest.fixture
def product_library():
    _lib.set_library_for_testing(None)      # default: promp_amd/libpromp_hip.so
    yield
    session._current = None


def run_plugin_scenario(algo_cls, O, A, hidden, M=3, P=4, T=40, Tmax=44, alpha=0.1, seed=7):
    """paths -> DiceMetaSampleProcessor -> algo._adapt -> paths at the adapted parameters -> processor -> algo.optimize_policy;
    the inner step and the parameters after the one Adam step against the oracle on the processor's own padded samples
    (as test_plugin_api.run_dice_maml_scenario compares them)"""
    from oracle import dice, policy as op, promp as pm
    from promp_amd import synthetic
    from promp_amd.baselines.linear_baseline import LinearFeatureBaseline, LinearTimeBaseline
    from promp_amd.meta_algos.vpg_dice_maml import VPG_DICEMAML
    from promp_amd.policies.meta_gaussian_mlp_policy import MetaGaussianMLPPolicy
    from promp_amd.samplers.dice_sample_processor import DiceMetaSampleProcessor
    from promp_amd.utils import logger
    logger.configure(quiet=True)
    vpg = algo_cls is VPG_DICEMAML
    rng = np.random.RandomState(seed)
    spec = op.PolicySpec(O, A, hidden)
    theta = synthetic.init_theta(rng, O, hidden, A)
    theta = (theta + 0.05 * rng.randn(theta.size)).astype(np.float32)
    t64 = theta.astype(np.float64)
    policy = MetaGaussianMLPPolicy(name='p', obs_dim=O, action_dim=A, meta_batch_size=M, hidden_sizes=hidden)
    policy.set_params(spec.to_ordered_dict(theta))
    proc = DiceMetaSampleProcessor(LinearTimeBaseline(), max_path_length=Tmax, discount=0.99, normalize_adv=True,
                                   **(dict(return_baseline=LinearFeatureBaseline(), gae_lambda=1.0) if vpg else {}))
    algo = algo_cls(Tmax, policy=policy, learning_rate=1e-3, inner_lr=alpha, meta_batch_size=M, num_inner_grad_steps=1)
    alpha64 = np.full(spec.n_params, alpha)
    policy.switch_to_pre_update()
    s0 = proc.process_samples(synthetic.make_paths(rng, np.tile(theta, (M, 1)), M, P, T, O, A, hidden, ragged=True), log=False)
    algo._adapt(s0)
    slabs0 = [dice.to_slab(dict(sd)) for sd in s0]
    ad = np.stack(dice.adapt(spec, [t64] * M, slabs0, alpha64))
    got = np.stack([spec.from_ordered_dict(d) for d in policy.policies_params_vals])
    assert np.max(np.abs((got - theta) - (ad - t64))) < 1e-4 * np.max(np.abs(ad - t64))
    s1 = proc.process_samples(synthetic.make_paths(rng, got, M, P, T, O, A, hidden, ragged=True), log=False)
    slabs1 = [dice.to_slab(dict(sd)) for sd in s1]
    algo.optimize_policy([s0, s1], log=False)
    r = dice.meta_objective_and_grad(spec, t64, [slabs0, slabs1], alpha64, outer='vpg' if vpg else 'dice')
    th_ref = pm.adam_step(t64, r['grad'], pm.AdamState(spec.n_params), 1e-3)
    # test_plugin_api.run_dice_maml_scenario holds the loss to 1e-6 on the register-chained kernels' fixture; here it gets the
    # bound every device loss gets against the float64 oracle (parity_checks: rtol 1e-4, atol 1e-6): the VPG-DiCE loss is a sum
    # over log-likelihoods from the split-arithmetic forward pass, and the DiCE loss is a float32 sum of baseline-subtracted
    # rewards, whose terms cancel
    print('plugin %s %s obs %d: loss_before %.9g  oracle %.9g' % (algo_cls.__name__, hidden, O, algo.last_stats['loss_before'], r['loss']))
    np.testing.assert_allclose(algo.last_stats['loss_before'], r['loss'], rtol=1e-4, atol=1e-6)
    got = spec.from_ordered_dict(policy.get_param_values())
    d_dev, d_ref = got - theta, th_ref - t64            # Adam's first step is lr * sign(g) wherever |g| >> eps
    assert np.mean(np.sign(d_dev) == np.sign(d_ref)) > 0.98 and np.max(np.abs(d_dev)) < 1.01e-3


@pytest.mark.parametrize('O,A,hidden', [(111, 8, (128, 128)), (20, 6, (64, 64, 64))])
def test_dice_maml_plugin(product_library, O, A, hidden):
    from promp_amd.meta_algos.dice_maml import DICEMAML
    run_plugin_scenario(DICEMAML, O, A, hidden)


def test_vpg_dice_maml_plugin(product_library):
    from promp_amd.meta_algos.vpg_dice_maml import VPG_DICEMAML
    run_plugin_scenario(VPG_DICEMAML, 111, 8, (128, 128))
