"""CPU: a dense matrix of scalar plaintexts times a batch (CKKSEncoder_EncodeScalars / _EncodeIntegerScalars, Evaluator_LiftScalars,
Evaluator_DotScalarsDevice; shl_dot_scalars) with the kernels emulated.  Exact word equality: against DotPlainMapped over the dense
map with expanded plaintexts, against the per-object forms on batches of one, against the REAL reference (oracle/_ref) where it is
built, and against Python-integer arithmetic around the flush interval and across the cuts.  (Capture and replay are in the GPU
suite only: the emulator does not replay graphs.)"""
import pytest


SCHEMES = ["ckks", "bfv", "bgv"]
# N = 8: every lane of a wave in another row; 64: a wave spans rows; 128: the first ring on the wave-uniform path; the last ring has
# both arithmetic classes (60- and 40-bit primes) in one level
RINGS = [(8, [30, 30, 30]), (64, [60, 40, 40, 60]), (128, [60, 40, 60]), (1024, [60, 40, 40, 60])]
SMALL = (1024, [60, 40, 60])
DEFERS = (8192, [50, 40, 40, 60])   # the smallest ring at which the library defers tails and products


def test_row_counts_come_from_the_tile(emu):
    import dot_scalars_cases as DS
    R, flush = DS.info()
    assert R in (2, 4, 8) and flush == 256
    assert DS.row_counts() == sorted({1, R - 1, R, R + 1, 2 * R + 1})


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", RINGS)
def test_parity(emu, scheme, n, bits):
    import dot_scalars_cases as DS
    DS.case_parity(scheme, n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_lowest_level(emu, scheme):
    """K = 1"""
    import dot_scalars_cases as DS
    DS.case_parity(scheme, *SMALL, sizes=(2,), ci=0)


def test_encode_scalars(emu):
    import dot_scalars_cases as DS
    DS.case_encode_scalars()


def test_encode_integer_scalars(emu):
    import dot_scalars_cases as DS
    DS.case_encode_integer_scalars()


@pytest.mark.parametrize("scheme", ["bfv", "bgv"])
@pytest.mark.parametrize("bits,tbits,fast", [([40, 40, 60], 20, True), ([30, 30, 60], 40, False)])
def test_lift_scalars(emu, scheme, bits, tbits, fast):
    """t below every prime (fast plain lift) and above them (the multi-precision lift)"""
    import dot_scalars_cases as DS
    DS.case_lift_scalars(scheme, 1024, bits, tbits, fast)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (64, [60, 40, 40, 60]), (128, [60, 40, 40, 60])])
def test_flush_boundaries(emu, n, bits):
    """per lane (N = 8, 64) and per wave (N = 128); 60-bit and 40-bit primes in one level"""
    import dot_scalars_cases as DS
    DS.case_flush(n, bits)


@pytest.mark.parametrize("row_tile", [2, 4, 8])
@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (128, [60, 40, 40, 60])])
def test_flush_boundaries_every_tile(emu, n, bits, row_tile):
    """every built row tile, per lane (N = 8) and per wave (N = 128): the accumulators carry the running residue across the flush"""
    import dot_scalars_cases as DS
    DS.case_flush(n, bits, batches=[DS.DOT_FLUSH - 1, DS.DOT_FLUSH, DS.DOT_FLUSH + 1, 2 * DS.DOT_FLUSH + 3], patterns=("max", "random"),
                  row_tile=row_tile)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (1024, [60, 40, 40, 60])])
def test_cuts(emu, n, bits):
    import dot_scalars_cases as DS
    DS.case_cuts(n, bits)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (128, [60, 40, 40, 60]), (1024, [60, 40, 40, 60])])
def test_every_built_tile(emu, n, bits):
    """R = 2, 4 and 8 on the per-lane and on the wave-uniform path"""
    import dot_scalars_cases as DS
    DS.case_tiles(n, bits)


def test_natural_slices(emu):
    import dot_scalars_cases as DS
    DS.case_natural_slices("ckks", *SMALL)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_out_of_place(emu, scheme):
    import dot_scalars_cases as DS
    DS.case_out_of_place(scheme, *DEFERS)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_transparent_check(emu, scheme):
    import dot_scalars_cases as DS
    DS.case_transparent_check(scheme, *DEFERS)


def test_pending_state(emu):
    import dot_scalars_cases as DS
    DS.case_pending(*DEFERS)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_errors(emu, scheme):
    import dot_scalars_cases as DS
    DS.case_errors(scheme, *SMALL)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_producer_errors(emu, scheme):
    import dot_scalars_cases as DS
    DS.case_producer_errors(scheme, *SMALL)
