"""tests/layered_checks.py's subset for the emulator (kernel sources on the SIMT interpreter, one OS thread per lane): a work item of
321 rows -- six rounds over the four splits of k_gb_linear, the second of split 1 with one row; eleven chunks of k_gb_wgrad, the last
with one row; two blocks of k_gen_loss -- and the shape whose every width is 1.  The conditions on the inputs of the GPU cases (a
dropped row must move the oracle's gradient by ten tolerances) are checked here, without any kernel."""
import pytest

from tests import devlib, layered_checks as lc

EMU_ROWS = [[300, 21]]                                  # row case C's 321-row task alone
# scalar loads over two chunks with a one-entry tail, NBW 1.  Nine actions keep the shape on the layer-by-layer kernels; with two it
# is padded onto the register-chained (64, 32) kernels, where the same item is 21 tiles on one workgroup's waves
EMU_SHAPES = {'h33x20_o5_a9': dict(hidden=(33, 20), O=5, A=9, layered=True), 'h33x20_o5_a2': dict(hidden=(33, 20), O=5, A=2, layered=False)}


@pytest.fixture(scope='module')
def lib():
    return devlib.emu_library()


@pytest.fixture
def one_cu(monkeypatch, lib):
    monkeypatch.setenv('PROMP_EMU_CUS', '2')      # fewer host threads per emulated launch
    lc.long_items(monkeypatch, lib, 1)


@pytest.mark.parametrize('shape', sorted(lc.ROW_SHAPES))
@pytest.mark.parametrize('case', sorted(lc.ROW_CASES))
def test_inputs_of_the_row_cases_show_a_dropped_row(case, shape):
    lc.check_inputs_show_a_dropped_row(case, shape)


@pytest.mark.parametrize('what', ['loss_grad', 'hvp'])
@pytest.mark.parametrize('shape', sorted(EMU_SHAPES))
def test_long_work_item(lib, one_cu, shape, what):
    lc.run_check(lib, 'emu rows 321 %s' % shape, what, 721, lc.shape_kwargs(EMU_ROWS, **EMU_SHAPES[shape]))


def test_every_width_one(lib, one_cu):
    c = lc.WIDTH_CASES['h1_o1_a1']
    lc.run_check(lib, 'emu width h1_o1_a1', 'loss_grad', 722, lc.shape_kwargs(**c))
    lc.run_check(lib, 'emu width h1_o1_a1', 'hvp', 722, lc.shape_kwargs(**c))
