"""CPU (fiber emulator): the BEHZ kernels of BFV multiplication at every dispatch class and at their bounds (behz_cases.py) - the
exact model against the oracle's stages, every steering target reached, and the emulated kernels word for word against both.
The device runs the same cases in test_gpu_behz.py."""
import pytest

import behz_cases as B


@pytest.mark.parametrize("name", B.ORDER + [B.STRIDE[0]])
def test_model_vs_oracle(name):
    B.case_model_vs_oracle(name)


@pytest.mark.parametrize("name", B.ORDER)
def test_classes(name):
    B.case_classes(name)


@pytest.mark.parametrize("name", B.THRESHOLD)
def test_threshold(emu, name):
    B.case_threshold(name)


@pytest.mark.parametrize("name", B.ORDER)
def test_stages(emu, name):
    B.case_stages(name)


@pytest.mark.parametrize("name", B.EVALUATOR)
def test_evaluator(emu, name):
    B.case_evaluator(name)


def test_evaluator_size3_times_size2(emu):
    B.case_evaluator_3x2()


@pytest.mark.parametrize("kernel", ["lift", "floor_sk", "stage"])
def test_stride(emu, kernel):
    B.case_stride(kernel)
