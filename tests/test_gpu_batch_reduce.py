"""GPU: sums over the items of a device-resident batch (Evaluator_SumItems / Evaluator_DotPlainDevice) on the gfx950 kernels:
N = 8192 (both arithmetic classes in one level), 32768, the C5 chain at N = 65536 once, the N = 8 ring and K = 1.  Against the REAL
reference (oracle/_ref) where it is built, against the per-object forms on batches of one, and against Python-integer arithmetic
around the flush intervals of the lazy accumulators."""
import pytest

import sealref

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not sealref.available(), reason="oracle/_ref (the real reference) is not built")

SCHEMES = ["ckks", "bfv", "bgv"]
C5 = (65536, [60] + [50] * 14 + [60])
MID = (8192, [60, 40, 40, 60])


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", [MID, (32768, [60, 50, 50, 50, 60])])
def test_parity(gpu, scheme, n, bits):
    """g = 1, 2 (two output items) and the whole batch"""
    import batch_reduce_cases as BR
    BR.case_parity(scheme, n, bits, batch=4, groups=(1, 2, 4))


@pytest.mark.parametrize("scheme", SCHEMES)
def test_group_not_a_power_of_two(gpu, scheme):
    """B = 15, g = 5: by the documented rule these launches are not cut, test_sliced and test_natural_slices cover the cut"""
    import batch_reduce_cases as BR
    BR.case_parity(scheme, *MID, batch=15, groups=(5,), sizes=(2,))


def test_parity_c5(gpu):
    import batch_reduce_cases as BR
    BR.case_parity("ckks", *C5, batch=3, groups=(3,), sizes=(2,))


@pytest.mark.parametrize("scheme", SCHEMES)
def test_lowest_level(gpu, scheme):
    """K = 1"""
    import batch_reduce_cases as BR
    BR.case_parity(scheme, *MID, batch=4, groups=(2, 4), sizes=(2,), ci=0)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_small_ring(gpu, scheme):
    import batch_reduce_cases as BR
    BR.case_parity(scheme, 8, [30, 30, 30], batch=4, groups=(1, 2, 4))


@pytest.mark.parametrize("group", [15, 16, 17, 255, 256, 257, 515])
def test_flush_boundaries(gpu, group):
    import batch_reduce_cases as BR
    assert group in BR.flush_groups()
    BR.case_flush(*MID, group, patterns=("max", "alternating", "half") if group > 17 else ("max", "alternating", "half", "random"))


def test_flush_boundaries_small_ring(gpu):
    import batch_reduce_cases as BR
    BR.case_flush(8, [30, 30, 30], 257, out_items=2)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_sliced(gpu, scheme):
    """a group of 23 items in 1, 2, 3, 4, 5 and 23 slices: most do not divide it"""
    import batch_reduce_cases as BR
    BR.case_sliced(scheme, *MID, batch=46, group=23, slice_counts=(2, 3, 4, 5, 23), size=2)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (1024, [60, 40, 60])])
def test_plane_counts(gpu, n, bits):
    """sizes 1, 4 and 5, in one launch and in two slices of a group of three"""
    import batch_reduce_cases as BR
    BR.case_plane_counts(n, bits)


def test_natural_slices(gpu):
    """N = 8192, K = 3: 12288 output pairs per item, so one group of 16 is cut and 11 of them are not (asserted inside)"""
    import batch_reduce_cases as BR
    BR.case_natural_slices("ckks", *MID, group=16)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_out_of_place(gpu, scheme):
    import batch_reduce_cases as BR
    BR.case_out_of_place(scheme, *MID)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_errors(gpu, scheme):
    import batch_reduce_cases as BR
    BR.case_errors(scheme, *MID)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_transparent_check(gpu, scheme):
    import batch_reduce_cases as BR
    BR.case_transparent_check(scheme, *MID)


def test_pending_state(gpu):
    import batch_reduce_cases as BR
    BR.case_pending(8192, [50, 40, 40, 60], batch=4, group=2)


def test_capture(gpu):
    """groups of 8 into two output items: by the documented rule the recorded dot product is cut and uses pool scratch"""
    import batch_reduce_cases as BR
    assert BR.rule_slices(2 * 3 * 8192 // 2, 8) == 2
    BR.case_capture(*MID, batch=16, group=8)


@needs_ref
def test_pipeline_ckks(gpu):
    import batch_reduce_cases as BR
    BR.case_pipeline_ckks(*MID, batch=5)


@needs_ref
def test_pipeline_bfv(gpu):
    import batch_reduce_cases as BR
    BR.case_pipeline_bfv(*MID, batch=5)
