"""MI355X: the BEHZ kernels of BFV multiplication at every dispatch class and at their bounds (behz_cases.py) - the fused kernels
and the staged ones word for word against the oracle's stages and the exact model, in ascending K so that a refused launch names
its size; through the Evaluator at one configuration per class; and past the capped grid."""
import pytest

import behz_cases as B

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", B.THRESHOLD)
def test_threshold(gpu, name):
    B.case_threshold(name)


@pytest.mark.parametrize("name", B.ORDER)
def test_stages(gpu, name):
    B.case_model_vs_oracle(name)
    B.case_classes(name)
    B.case_stages(name)


@pytest.mark.parametrize("name", B.EVALUATOR)
def test_evaluator(gpu, name):
    B.case_evaluator(name)


def test_evaluator_size3_times_size2(gpu):
    B.case_evaluator_3x2()


@pytest.mark.parametrize("kernel", ["lift", "floor_sk", "stage"])
def test_stride(gpu, kernel):
    B.case_stride(kernel)
