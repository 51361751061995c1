"""tests/count_axis_checks.py's subset for the emulator (kernel sources on the SIMT interpreter, one OS thread per lane): eight inner
steps on the register-chained kernels, four on the layer-by-layer ones, 49 tasks -- the second trip of the final stage's column sum,
one task in it -- and the refusal of a ninth step.  Indexing and host sequencing only: what a second trip or a ninth slab can get
wrong on hardware is test_gpu_count_axes.py's."""
import pytest

from tests import count_axis_checks as cc, devlib


@pytest.fixture(scope='module')
def lib():
    return devlib.emu_library()


@pytest.fixture(autouse=True)
def few_host_threads(monkeypatch):
    monkeypatch.setenv('PROMP_EMU_CUS', '2')      # fewer host threads per emulated launch
    for name in ('PROMP_MAX_CUS', 'PROMP_WIDE_FP32', 'PROMP_GEN_FP32'):
        monkeypatch.delenv(name, raising=False)


def test_eight_inner_steps_on_the_chain_kernels(lib):
    cc.check_meta_k(lib, 'chain', 8)


def test_four_inner_steps_layer_by_layer(lib):
    cc.check_meta_k(lib, 'layered', 4, epochs=1)


def test_49_tasks_take_a_second_trip_of_the_column_sum(lib):
    cc.check_meta_m(lib, 49, epochs=1)


def test_nine_inner_steps_are_refused(lib):
    cc.check_refused_k(lib)
