"""GPU: a matrix of scalar weights times a matrix of ciphertexts (Evaluator_MatMulScalarsItems; shl_matmul_scalars) on the gfx950
kernel, wide ([K] words per weight) and narrow (one signed 32-bit integer per weight): the N = 8 and N = 64 rings (weights loaded
per lane), N = 128 (the first ring where a wave stays in its row and the weights are scalar loads), N = 8192 (both arithmetic
classes in one level), K = 1 and the C5 chain at N = 65536 once.  Exact word equality and the metadata triple: against
MatMulPlainItems on the expanded plaintexts, DotScalarsDevice at one column, the per-object forms and the REAL reference
(oracle/_ref) where it is built, and against Python-integer arithmetic around both flush intervals, across the cuts and for every
built row tile."""
import pytest

pytestmark = pytest.mark.gpu

SCHEMES = ["ckks", "bgv", "bfv"]
C5 = (65536, [60] + [50] * 14 + [60])
MID = (8192, [60, 40, 40, 60])
RINGS = [(8, [30, 30, 30]), (64, [60, 40, 40, 60]), (128, [60, 40, 60]), MID]
DEFERS = (8192, [50, 40, 40, 60])


def test_shapes_come_from_the_tile(gpu):
    import matmul_scalars_cases as MS
    R, Rn, flush, nflush = MS.info()
    assert R in MS.TILES and Rn in MS.TILES and (flush, nflush) == (256, 1024)
    assert MS.row_counts(R) == sorted({1, R - 1, R, R + 1, 2 * R + 1})
    assert {r for r, _ in MS.shapes(R)} == set(MS.row_counts(R)) and {c for _, c in MS.shapes(R)} == {1, 2, 3}


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", RINGS)
def test_parity(gpu, scheme, n, bits):
    import matmul_scalars_cases as MS
    MS.case_parity(scheme, n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_lowest_level(gpu, scheme):
    """K = 1"""
    import matmul_scalars_cases as MS
    MS.case_parity(scheme, *MID, sizes=(2,), ci=0)


def test_parity_c5(gpu):
    """rows 3, inner 2, cols 2 against MatMulPlainItems only"""
    import matmul_scalars_cases as MS
    MS.case_parity("ckks", *C5, sizes=(2,), inner=2, shape_list=[(3, 2)], per_object=False)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", [(8, [40, 40, 40]), (128, [60, 40, 60]), MID])
def test_narrow_equals_wide(gpu, scheme, n, bits):
    import matmul_scalars_cases as MS
    MS.case_narrow_equals_wide(scheme, n, bits)


@pytest.mark.parametrize("narrow", [False, True])
@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (128, [60, 40, 40, 60])])
def test_flush_boundaries(gpu, n, bits, narrow):
    import matmul_scalars_cases as MS
    MS.case_flush(n, bits, narrow)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), MID])
def test_cuts(gpu, n, bits):
    import matmul_scalars_cases as MS
    MS.case_cuts("ckks", n, bits)


def test_natural_slices(gpu):
    import matmul_scalars_cases as MS
    MS.case_natural_slices("bgv", *MID)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (128, [60, 40, 40, 60])])
def test_every_built_tile(gpu, n, bits):
    """the per-lane and the wave-uniform path"""
    import matmul_scalars_cases as MS
    MS.case_tiles(n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_out_of_place(gpu, scheme):
    import matmul_scalars_cases as MS
    MS.case_out_of_place(scheme, *DEFERS)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_transparent_check(gpu, scheme):
    import matmul_scalars_cases as MS
    MS.case_transparent_check(scheme, *DEFERS)


def test_pending_state(gpu):
    import matmul_scalars_cases as MS
    MS.case_pending(*DEFERS)


@pytest.mark.parametrize("narrow", [False, True])
def test_capture(gpu, narrow):
    """inner = 16 at R x 3: by the documented rule the recorded call is cut and uses pool scratch (asserted inside)"""
    import matmul_scalars_cases as MS
    MS.case_capture(*MID, narrow)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_errors(gpu, scheme):
    import matmul_scalars_cases as MS
    MS.case_errors(scheme, *DEFERS)
