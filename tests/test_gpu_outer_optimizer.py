"""The outer optimiser on the MI355X (tests/outer_optimizer_checks.py): every rule against its float64 mirror on the device's own
inputs, the general final-stage kernels against the plain ones bit for bit, the clip by the global norm inactive and active,
every route to a step against the others, end to end against the float64 oracle, and the plugins.  The shapes are the smallest at
which each path can go wrong: M 3 on the chain kernels, M 5 (five tasks over four task quarters) for the split stage, K 2 with
(64, 64), and (48, 20) zero-padded on (64, 32)."""
import pytest

from promp_amd import _lib, session
from tests import devlib, outer_optimizer_checks as oc, step_size_checks as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    return devlib.gpu_library()


@pytest.fixture(scope='module')
def shape1():
    return sc.PrompCase(711, M=3, P=2, T=50, O=7, A=3, hidden=(32, 32), K=1, ragged=True)


@pytest.fixture(scope='module')
def shape5():                 # five tasks over four task quarters: final_quarter_sum's tail
    return sc.PrompCase(712, M=5, P=2, T=50, O=7, A=3, hidden=(32, 32), K=1, ragged=True)


@pytest.fixture(scope='module')
def shape2():
    return sc.PrompCase(713, M=3, P=2, T=50, O=20, A=6, hidden=(64, 64), K=2, ragged=True)


@pytest.fixture(scope='module')
def padded():
    return sc.PrompCase(714, M=3, P=2, T=50, O=20, A=6, hidden=(48, 20), K=1)


@pytest.fixture
def product_library():
    _lib.set_library_for_testing(None)
    yield
    session._current = None


@pytest.mark.parametrize('clip', [False, True])
@pytest.mark.parametrize('key', sorted(oc.RULES))
def test_rule_against_its_mirror(lib, shape1, key, clip):
    oc.check_rule(lib, shape1, key, clip)


@pytest.mark.parametrize('key', sorted(oc.RULES))
def test_rule_with_learn_std_false(lib, shape1, key):
    oc.check_rule(lib, shape1, key, clip=True, learn_std=False)


@pytest.mark.parametrize('key', sorted(oc.RULES))
def test_rule_with_trained_step_sizes(lib, shape5, key):
    oc.check_rule(lib, shape5, key, clip=True, sizes=True)
    oc.check_rule(lib, shape5, key, clip=False, sizes=True, learn_std=False, steps=2)


@pytest.mark.parametrize('key', sorted(oc.RULES))
def test_rule_two_inner_steps_and_zero_padded_widths(lib, shape2, padded, key):
    oc.check_rule(lib, shape2, key, clip=True, steps=2)
    # (48, 20) on the (64, 32) kernels: the norm the device reports is the caller-layout norm -- the padding adds nothing
    oc.check_rule(lib, padded, key, clip=True, sizes=True, steps=2)


def test_forced_general_kernels_equal_the_plain_ones(lib, shape5, monkeypatch):
    oc.check_generic_equals_plain(lib, shape5, monkeypatch)


def test_forced_general_kernels_equal_the_plain_ones_padded(lib, padded, monkeypatch):
    oc.check_generic_equals_plain(lib, padded, monkeypatch)


def test_inactive_clip_is_no_clip(lib, shape5, shape2):
    oc.check_inactive_clip(lib, shape5)
    oc.check_inactive_clip(lib, shape5, sizes=True)
    oc.check_inactive_clip(lib, shape2)


def test_adam_arguments_against_the_oracle(lib, shape1):
    oc.check_adam_arguments(lib, shape1)


@pytest.mark.parametrize('clip', [False, True])
@pytest.mark.parametrize('key', ['sgd', 'momentum'])
def test_linear_rules_against_the_oracle(lib, shape1, key, clip):
    oc.check_linear_rule(lib, shape1, key, clip)


def test_routes_agree_with_clipping_on(lib, shape5):
    oc.check_routes_with_clip(lib, shape5, 'adam', sizes=True)
    oc.check_routes_with_clip(lib, shape5, 'nesterov', comm=False)
    oc.check_routes_with_clip(lib, shape5, 'sgd', comm=False)


# The final stage's grid edges (outer_optimizer_checks.EDGE_SHAPES: Theta 60, 62, 255, 256; M 2 or 5, 20 to 100 rows): the scalar
# columns across a column block's edge, exactly full reduce grids, the statistics thread on a thread block's edge.
EDGES = sorted(oc.EDGE_SHAPES)


@pytest.mark.parametrize('edge', EDGES)
def test_final_stage_edges_split_equals_fused(lib, edge):
    sc.check_split_equals_fused(lib, oc.edge_case(edge))


@pytest.mark.parametrize('edge', EDGES)
def test_final_stage_edges_general_equals_plain(lib, edge, monkeypatch):
    oc.check_generic_equals_plain(lib, oc.edge_case(edge), monkeypatch)


@pytest.mark.parametrize('edge', EDGES)
def test_final_stage_edges_rules(lib, edge):
    oc.check_rule(lib, oc.edge_case(edge), 'adam', clip=True, sizes=True)
    oc.check_rule(lib, oc.edge_case(edge), 'nesterov', clip=False)


@pytest.mark.parametrize('edge', EDGES)
def test_final_stage_edges_routes_with_clip(lib, edge):
    oc.check_routes_with_clip(lib, oc.edge_case(edge), 'adam', sizes=True)


@pytest.mark.parametrize('edge', EDGES)
def test_final_stage_edges_statistics_against_the_exchange_buffer(lib, edge):
    oc.check_stats_against_exchange(lib, oc.edge_case(edge))


def test_minibatched_sgd_with_clip_equals_truncated_batches(lib):
    oc.check_minibatch_sgd_clip(lib, 715)


def test_state(lib, shape1):
    oc.check_state(lib, shape1)
    oc.check_session_keeps_settings(lib)


def test_refusals(lib, shape1):
    oc.check_refusals(lib, shape1)


def test_promp_plugin_clips_logs_and_snapshots(product_library, tmp_path):
    oc.check_promp_plugin(str(tmp_path / 'snap'))


@pytest.mark.parametrize('algo', ['vpg', 'dice'])
def test_other_plugins_under_sgd(product_library, algo):
    oc.check_other_plugin(algo)
