"""GPU: item maps (ItemMap_Create; Evaluator_SumItemsMapped / DotPlainMapped / DotItemsMapped; shl_reduce_mapped) on the gfx950
kernels: the N = 8 and N = 64 rings (per-lane walk), N = 128 (the first ring on the wave-uniform walk), N = 8192 (both arithmetic
classes in one level), K = 1 and the C5 chain at N = 65536 once.  Against the REAL reference (oracle/_ref) where it is built,
against the per-object forms on batches of one holding the named items, and against Python-integer arithmetic around the flush
intervals and across the cuts."""
import pytest

import sealref

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not sealref.available(), reason="oracle/_ref (the real reference) is not built")

SCHEMES = ["ckks", "bfv", "bgv"]
C5 = (65536, [60] + [50] * 14 + [60])
MID = (8192, [60, 40, 40, 60])
RINGS = [(8, [30, 30, 30]), (64, [60, 40, 40, 60]), (128, [60, 40, 60]), MID]


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", RINGS)
def test_parity(gpu, scheme, n, bits):
    import item_map_cases as IM
    IM.case_parity(scheme, n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_lowest_level(gpu, scheme):
    """K = 1"""
    import item_map_cases as IM
    IM.case_parity(scheme, *MID, sizes=(2,), ci=0)


def test_parity_c5(gpu):
    """a 3-item source: a single and a row with a repeat"""
    import item_map_cases as IM
    IM.case_parity("ckks", *C5, sizes=(2,), source=3, rows=[[2], [0, 1, 1]], second=[[1], [0, 0, 1]], second_same=[[0], [2, 1, 0]])


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", [RINGS[0], MID])
def test_gather(gpu, scheme, n, bits):
    import item_map_cases as IM
    IM.case_gather(scheme, n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_identity_map_is_the_contiguous_form(gpu, scheme):
    """B = 15, g = 5"""
    import item_map_cases as IM
    IM.case_identity(scheme, *MID)


@pytest.mark.parametrize("n,bits,patterns", [(8, [30, 30, 30], None), (64, [60, 40, 40, 60], None), (8192, [60, 40, 40, 60], ("max",))])
def test_ragged_flush_boundaries(gpu, n, bits, patterns):
    import item_map_cases as IM
    IM.case_flush(n, bits, **({} if patterns is None else {"patterns": patterns}))


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (1024, [60, 40, 60])])
def test_ragged_cuts(gpu, n, bits):
    import item_map_cases as IM
    IM.case_cuts(n, bits)


def test_natural_slices(gpu):
    """N = 8192, K = 3: 49152 output pairs for four rows - the map of mean row 10 is cut, the one of mean row 5 is not"""
    import item_map_cases as IM
    IM.case_natural_slices(*MID)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_out_of_place(gpu, scheme):
    import item_map_cases as IM
    IM.case_out_of_place(scheme, *MID)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_transparent_check(gpu, scheme):
    import item_map_cases as IM
    IM.case_transparent_check(scheme, *MID)


def test_pending_state(gpu):
    import item_map_cases as IM
    IM.case_pending(8192, [50, 40, 40, 60])


def test_capture(gpu):
    """rows of 16 and 12 terms: by the documented rule the recorded products are cut and use pool scratch (asserted inside)"""
    import item_map_cases as IM
    IM.case_capture(*MID)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_map_destroyed_after_the_call(gpu, scheme):
    import item_map_cases as IM
    IM.case_destroy_after_call(scheme, *MID)


def test_create_errors(gpu):
    import item_map_cases as IM
    IM.case_create_errors("ckks", *MID)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_errors(gpu, scheme):
    import item_map_cases as IM
    IM.case_errors(scheme, *MID)


@needs_ref
def test_pipeline_sparse_matrix(gpu):
    import item_map_cases as IM
    IM.case_pipeline_sparse_matrix(*MID)


@needs_ref
def test_pipeline_pairs(gpu):
    import item_map_cases as IM
    IM.case_pipeline_pairs(*MID)
