"""CPU: a matrix of scalar weights times a matrix of ciphertexts (Evaluator_MatMulScalarsItems; shl_matmul_scalars) with the kernels
emulated, wide ([K] words per weight) and narrow (one signed 32-bit integer per weight).  Exact word equality and the metadata
triple: against MatMulPlainItems on the expanded plaintexts, DotScalarsDevice at one column, the per-object forms and the REAL
reference (oracle/_ref) where it is built, and against Python-integer arithmetic around both flush intervals, across the cuts and
for every built row tile.  (Capture and replay are in the GPU suite only: the emulator does not replay graphs.)"""
import pytest


SCHEMES = ["ckks", "bgv", "bfv"]
# N = 8 and 64: the lanes of a wave in different rows of the grid, weights loaded per lane; 128: the first ring where a wave stays in
# its row and the weights are scalar loads; the last ring has both arithmetic classes (60- and 40-bit primes) in one level
MID = (1024, [60, 40, 40, 60])
RINGS = [(8, [30, 30, 30]), (64, [60, 40, 40, 60]), (128, [60, 40, 60]), MID]
DEFERS = (8192, [50, 40, 40, 60])   # the smallest ring at which the library defers tails and products


def test_shapes_come_from_the_tile(emu):
    import matmul_scalars_cases as MS
    R, Rn, flush, nflush = MS.info()
    assert R in MS.TILES and Rn in MS.TILES and (flush, nflush) == (256, 1024)
    assert MS.row_counts(R) == sorted({1, R - 1, R, R + 1, 2 * R + 1})
    assert {r for r, _ in MS.shapes(R)} == set(MS.row_counts(R)) and {c for _, c in MS.shapes(R)} == {1, 2, 3}


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", RINGS)
def test_parity(emu, scheme, n, bits):
    import matmul_scalars_cases as MS
    MS.case_parity(scheme, n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_lowest_level(emu, scheme):
    """K = 1"""
    import matmul_scalars_cases as MS
    MS.case_parity(scheme, *MID, sizes=(2,), ci=0)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", [(8, [40, 40, 40]), (128, [60, 40, 60]), MID])
def test_narrow_equals_wide(emu, scheme, n, bits):
    import matmul_scalars_cases as MS
    MS.case_narrow_equals_wide(scheme, n, bits)


@pytest.mark.parametrize("narrow", [False, True])
@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (128, [60, 40, 40, 60])])
def test_flush_boundaries(emu, n, bits, narrow):
    import matmul_scalars_cases as MS
    MS.case_flush(n, bits, narrow)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), MID])
def test_cuts(emu, n, bits):
    import matmul_scalars_cases as MS
    MS.case_cuts("ckks", n, bits)


def test_natural_slices(emu):
    import matmul_scalars_cases as MS
    MS.case_natural_slices("bgv", *MID)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (128, [60, 40, 40, 60])])
def test_every_built_tile(emu, n, bits):
    """the per-lane and the wave-uniform path"""
    import matmul_scalars_cases as MS
    MS.case_tiles(n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_out_of_place(emu, scheme):
    import matmul_scalars_cases as MS
    MS.case_out_of_place(scheme, *DEFERS)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_transparent_check(emu, scheme):
    import matmul_scalars_cases as MS
    MS.case_transparent_check(scheme, *DEFERS)


def test_pending_state(emu):
    import matmul_scalars_cases as MS
    MS.case_pending(*DEFERS)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_errors(emu, scheme):
    import matmul_scalars_cases as MS
    MS.case_errors(scheme, *DEFERS)
