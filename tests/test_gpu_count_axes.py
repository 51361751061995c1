"""tests/count_axis_checks.py on the MI355X: four and eight inner steps on every pass-kernel family and under every feature layered on
top (trained step sizes, DiCE, minibatches, the primal cache, adapt reuse, the constraint products and the CG solve, the split
route), and meta-batches of 48, 49 and 97 tasks (one, two and three trips of the final stage's column sum) and of n_cus + 1 and
2 n_cus + 1 tasks (every task floored to one work item, tables close to max_work, grids of M workgroups).  Tolerances are the reused
checks' own; profiles/count_axes.txt keeps one run's worst figures."""
import pytest

from tests import count_axis_checks as cc, devlib, minibatch_checks as mb, outer_optimizer_checks as oc, parity_checks as pc
from tests import point_collect_checks as gc, rollout_checks as rc, step_size_checks as sc

pytestmark = pytest.mark.gpu

SHAPES = sorted(cc.K_SHAPES)


@pytest.fixture(scope='module')
def lib():
    return devlib.gpu_library()


@pytest.fixture(autouse=True)
def default_plan(monkeypatch):
    for name in ('PROMP_MAX_CUS', 'PROMP_WIDE_FP32', 'PROMP_GEN_FP32'):
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope='module')
def n_cus(lib):
    return cc.device_cus(lib)


# ---- K ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('K', cc.K_VALUES)
@pytest.mark.parametrize('shape', SHAPES)
def test_meta_objective_through_k_inner_steps(lib, shape, K):
    cc.check_inputs_tell_the_steps_apart(shape, K)
    cc.check_meta_k(lib, shape, K)


def test_primal_cache_of_nine_slabs(lib):
    cc.check_primal_cache_k(lib, 8)


def test_adapt_reuse_through_eight_steps(lib):
    pc.check_adapt_reuse(lib, cc.k_seed('chain', 8), K=8, **cc.ragged_kwargs('chain'))


def test_schedule_invariance_through_eight_steps(lib):
    pc.check_schedule_invariance(lib, cc.k_seed('chain', 8), K=8, **cc.ragged_kwargs('chain'))


def test_constraint_product_through_four_steps(lib):
    pc.check_exact_constraint_hvp(lib, cc.k_seed('chain', 4), K=4, **cc.ragged_kwargs('chain'))


def test_cg_solve_mirror_through_four_steps(lib):
    seen = pc.check_cg_solve_mirror(lib, cc.k_seed('chain', 4), K=4, modes=(2,), iters=(3,), regs=(0.0,), freeze=False, zero_rhs=False,
                                    **cc.ragged_kwargs('chain'))
    assert seen == {(2, 3, 0.0): 3}


def test_dice_objectives_through_four_coupled_steps(lib):
    cc.check_dice_k(lib, 4)


def test_step_size_gradient_through_four_steps(lib):
    sc.check_alpha_grad(lib, cc.step_size_case(4))


def test_trained_step_sizes_split_route_through_four_steps(lib):
    sc.check_split_equals_fused(lib, cc.step_size_case(4))


def test_minibatches_through_four_steps(lib):
    mb.check_equals_truncated_batch(lib, cc.k_seed('chain', 4), 4, 2, (32, 32), 4)


def test_nine_inner_steps_are_refused(lib):
    cc.check_refused_k(lib)


# ---- M: the final stage's 48-task trips -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('M', cc.M_TRIPS)
def test_meta_objective_over_final_stage_trips(lib, M):
    cc.check_inputs_show_a_left_out_task(M)
    cc.check_meta_m(lib, M)


@pytest.mark.parametrize('M', cc.M_TRIPS)
def test_statistics_and_exchange_over_final_stage_trips(lib, M):
    oc.check_stats_against_exchange(lib, cc.task_case(M))


@pytest.mark.parametrize('M', cc.M_TRIPS)
def test_trained_step_sizes_split_route_over_final_stage_trips(lib, M):
    sc.check_split_equals_fused(lib, cc.task_case(M))


@pytest.mark.parametrize('M', cc.M_TRIPS)
def test_forced_general_final_stage_over_final_stage_trips(lib, M, monkeypatch):
    oc.check_generic_equals_plain(lib, cc.task_case(M), monkeypatch)


def test_three_minibatches_of_49_tasks(lib):
    cc.check_minibatches_m(lib, 49, 3)


# ---- M: more tasks than compute units --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('times', (1, 2))
@pytest.mark.parametrize('shape', SHAPES)
def test_every_family_with_more_tasks_than_units(lib, n_cus, shape, times):
    M = times * n_cus + 1
    cc.check_inputs_show_a_left_out_task(M, shape)
    cc.check_family_m(lib, shape, M, n_cus)


@pytest.mark.parametrize('times', (1, 2))
def test_cg_solve_with_more_tasks_than_units(lib, n_cus, times):
    M = times * n_cus + 1
    pc.check_cg_solve_on_device(lib, cc.m_seed(M), M=M, P=1, T=12, O=4, A=2, hidden=(32, 32), cg_iters=3)


@pytest.mark.parametrize('noise', ('host', 'device'))
@pytest.mark.parametrize('times', (1, 2))
def test_point_rollout_with_more_tasks_than_units(lib, n_cus, times, noise):
    rc.check_point_rollout(lib, times * n_cus + 1, 1, 3, (32, 32), 'dense', 0, noise, step=1, seed=rc.SEED64)


@pytest.mark.parametrize('times', (1, 2))
def test_policy_step_with_more_tasks_than_units(lib, n_cus, times):
    rc.check_policy_step(lib, times * n_cus + 1, 1, 2, 4, 2, (32, 32), layout='fixed', step=0, seed=rc.SEED31, clip_infos=True)


@pytest.mark.parametrize('times', (1, 2))
def test_policy_forward_with_more_tasks_than_units(lib, n_cus, times):
    rc.check_policy_forward(lib, times * n_cus + 1, 3, 4, 2, (32, 32))


def test_goal_collection_with_more_tasks_than_units(lib, n_cus):
    gc.check_goal_collect(lib, **cc.goal_collect_args(n_cus + 1))
