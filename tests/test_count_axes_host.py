"""The conditions on the inputs of tests/count_axis_checks.py, on the float64 oracle alone (no kernel): the inner KLs and their
coefficients tell the K steps apart, a task left out of the mean shows in the meta-gradient, every shape sits on the family it is
meant for, and the restated table counts are build_step_tables' own on the layouts tests/host/plan_check.cpp pins."""
import numpy as np
import pytest

from tests import count_axis_checks as cc, helpers

N_CUS = 256          # the MI355X: the task counts test_gpu_count_axes.py derives from the device


def test_eta_for_keeps_the_existing_coefficients_and_goes_on_to_eight():
    assert [helpers.eta_for(K).tolist() for K in (1, 2, 3)] == [np.array(v, np.float32).tolist() for v in ([5e-4], [5e-4, 1e-3], [5e-4, 1e-3, 2e-3])]
    for K in range(1, helpers.ETA_MAX + 1):
        eta = helpers.eta_for(K)
        assert eta.dtype == np.float32 and eta.shape == (K,) and len(set(eta.tolist())) == K
        assert np.array_equal(eta, helpers.eta_for(helpers.ETA_MAX)[:K])
    with pytest.raises(AssertionError):
        helpers.eta_for(helpers.ETA_MAX + 1)


@pytest.mark.parametrize('K', cc.K_VALUES)
@pytest.mark.parametrize('shape', sorted(cc.K_SHAPES))
def test_inner_kls_and_coefficients_tell_the_steps_apart(monkeypatch, shape, K):
    monkeypatch.delenv('PROMP_WIDE_FP32', raising=False)
    cc.check_inputs_tell_the_steps_apart(shape, K)


def test_step_size_references_agree_through_four_steps(monkeypatch):
    from tests import step_size_checks as sc
    monkeypatch.delenv('PROMP_WIDE_FP32', raising=False)
    sc.check_references(cc.step_size_case(4))


def test_dice_inputs_through_four_steps_can_be_judged_in_float32(monkeypatch):
    monkeypatch.delenv('PROMP_WIDE_FP32', raising=False)
    cc.check_dice_inputs(4)


@pytest.mark.parametrize('M,shape',[(M, cc.M_SHAPE) for M in cc.M_TRIPS] + [(M, s) for M in (N_CUS + 1, 2 * N_CUS + 1) for s in sorted(cc.K_SHAPES)])
def test_a_left_out_task_shows_in_the_meta_gradient(monkeypatch, M, shape):
    monkeypatch.delenv('PROMP_WIDE_FP32', raising=False)
    lens = [n for task in cc.m_lengths(M) for n in task]
    assert len(lens) == M and min(lens) >= 1 and max(lens) <= 20
    cc.check_inputs_show_a_left_out_task(M, shape)


def test_restated_table_counts_are_the_planners():
    # tests/host/plan_check.cpp: fused rows D and E at two units, A at one, and 257 one-tile tasks on 256 units
    assert cc.planned_counts([100, 100, 100], 2) == dict(items0=3, items1=4, segments=4, workgroups=2)
    assert cc.planned_counts([513], 2) == dict(items0=2, items1=4, segments=2, workgroups=2)
    assert cc.planned_counts([16, 17, 65, 80], 1) == dict(items0=4, items1=4, segments=4, workgroups=1)
    assert cc.planned_counts([16] * 257, 256) == dict(items0=257, items1=257, segments=257, workgroups=129)


@pytest.mark.parametrize('M', (N_CUS + 1, 2 * N_CUS + 1))
def test_tables_of_more_tasks_than_units_fit(M):
    c = cc.check_tables_fit(M, N_CUS)
    assert c['items0'] == M            # one workgroup per task on the cooperative kernels: nothing left to share out


def test_goal_collection_of_257_tasks_meets_its_events():
    from tests import point_collect_checks as gc
    gc.goal_case_is_sound(**cc.goal_collect_args(N_CUS + 1))
