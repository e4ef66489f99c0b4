"""CPU: a sparse matrix of scalar weights times a batch over an item map (Evaluator_DotScalarsMapped; shl_dot_scalars_mapped) with
the kernels emulated, wide ([K] words per weight) and narrow (one signed 32-bit integer per weight).  Exact word equality and the
metadata triple: against DotPlainMapped with the same map on the expanded plaintexts, DotScalarsDevice over the dense map,
Conv2dScalarsItems over the map of the in-image taps, the per-object forms and the REAL reference (oracle/_ref) where it is built,
and against Python-integer arithmetic for the shapes only this call has, around both flush intervals and across the cuts.
(Capture and replay are in the GPU suite only: the emulator does not replay graphs.)"""
import pytest


SCHEMES = ["ckks", "bgv", "bfv"]
# N = 8 and 64: the lanes of a wave in rows of different length, lists and weights loaded per lane; 128: the first ring where a wave
# stays in its row and lists and weights are scalar loads; the last ring has both arithmetic classes (60- and 40-bit primes) in one level
MID = (256, [60, 40, 40, 60])
RINGS = [(8, [30, 30, 30]), (64, [60, 40, 40, 60]), (128, [60, 40, 60]), MID]
DEFERS = (8192, [50, 40, 40, 60])   # the smallest ring at which the library defers tails and products


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", RINGS)
def test_parity(emu, scheme, n, bits):
    import dot_scalars_mapped_cases as DM
    DM.case_parity(scheme, n, bits, per_object=(n, bits) == MID)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_lowest_level(emu, scheme):
    """K = 1"""
    import dot_scalars_mapped_cases as DM
    DM.case_parity(scheme, *MID, sizes=(2,), ci=0, per_object=False)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), MID])
def test_dense_map_is_dot_scalars_device(emu, scheme, n, bits):
    import dot_scalars_mapped_cases as DM
    DM.case_dense(scheme, n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), MID])
def test_tap_map_is_conv2d(emu, scheme, n, bits):
    import dot_scalars_mapped_cases as DM
    DM.case_conv(scheme, n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (128, [60, 40, 60]), MID])
def test_depthwise_dilated_pooling(emu, scheme, n, bits):
    import dot_scalars_mapped_cases as DM
    DM.case_only_here(scheme, n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", [(8, [40, 40, 40]), (128, [60, 40, 60]), MID])
def test_narrow_equals_wide(emu, scheme, n, bits):
    import dot_scalars_mapped_cases as DM
    DM.case_narrow_equals_wide(scheme, n, bits)


@pytest.mark.parametrize("narrow", [False, True])
@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (128, [60, 40, 40, 60])])
def test_flush_boundaries(emu, n, bits, narrow):
    import dot_scalars_mapped_cases as DM
    DM.case_flush(n, bits, narrow)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), MID])
def test_cuts(emu, n, bits):
    import dot_scalars_mapped_cases as DM
    DM.case_cuts(n, bits)


def test_natural_slices(emu):
    import dot_scalars_mapped_cases as DM
    DM.case_natural_slices(*MID)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (128, [60, 40, 60])])
def test_untouched_neighbours(emu, n, bits):
    import dot_scalars_mapped_cases as DM
    DM.case_neighbours("bfv", n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_out_of_place(emu, scheme):
    import dot_scalars_mapped_cases as DM
    DM.case_out_of_place(scheme, *DEFERS)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_transparent_check(emu, scheme):
    import dot_scalars_mapped_cases as DM
    DM.case_transparent_check(scheme, *DEFERS)


def test_pending_state(emu):
    import dot_scalars_mapped_cases as DM
    DM.case_pending(*DEFERS)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_destroy_after_call(emu, scheme):
    import dot_scalars_mapped_cases as DM
    DM.case_destroy_after_call(scheme, *MID)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_errors(emu, scheme):
    import dot_scalars_mapped_cases as DM
    DM.case_errors(scheme, *DEFERS)
