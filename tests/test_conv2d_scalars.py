"""CPU: a 2-D convolution of scalar weights over a grid of ciphertexts (Evaluator_Conv2dScalarsItems; shl_conv2d_scalars) with the
kernels emulated, wide ([K] words per weight) and narrow (one signed 32-bit integer per weight).  Exact word equality and the
metadata triple: against DotPlainMapped over the map of the taps inside the image on the expanded plaintexts, MatMulScalarsItems
where the shape degenerates, the per-object forms and the REAL reference (oracle/_ref) where it is built, and against Python-integer
arithmetic around both flush intervals, across the cuts and for every built row tile and hint.  (Capture and replay are in the GPU
suite only: the emulator does not replay graphs.)"""
import pytest


SCHEMES = ["ckks", "bgv", "bfv"]
# N = 8 and 64: the lanes of a wave at different output positions, weights loaded per lane; 128: the first ring where a wave stays at
# its position and the weights are scalar loads; the last ring has both arithmetic classes (60- and 40-bit primes) in one level
MID = (256, [60, 40, 40, 60])
RINGS = [(8, [30, 30, 30]), (64, [60, 40, 40, 60]), (128, [60, 40, 60]), MID]
DEFERS = (8192, [50, 40, 40, 60])   # the smallest ring at which the library defers tails and products


def test_shape_list(emu):
    import conv2d_scalars_cases as CV
    import matmul_scalars_cases as MS
    for narrow in (False, True):
        R = MS.row_tile(narrow)
        got = CV.shapes(R)
        assert len(got) == 7 and {s.out_channels for s in got} == set(MS.row_counts(R))
    assert CV.shape_of(CV.ASYMMETRIC, 1).out_size() == (3, 7)
    s = CV.shape_of(CV.REMAINDER, 1)
    assert s.out_size() == (3, 2) and (s.height + 2 * s.pad_h - s.kernel_h) % s.stride_h and (s.width + 2 * s.pad_w - s.kernel_w) % s.stride_w
    assert sorted({len(r) for r in CV.tap_rows(CV.shape_of(CV.SAME_3X3, 1))}) == [8, 12, 18], "corner, edge, interior"


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", RINGS)
def test_parity(emu, scheme, n, bits):
    import conv2d_scalars_cases as CV
    CV.case_parity(scheme, n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_lowest_level(emu, scheme):
    """K = 1"""
    import conv2d_scalars_cases as CV
    CV.case_parity(scheme, *MID, sizes=(2,), ci=0, per_object=False)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", [(8, [40, 40, 40]), (128, [60, 40, 60]), MID])
def test_narrow_equals_wide(emu, scheme, n, bits):
    import conv2d_scalars_cases as CV
    CV.case_narrow_equals_wide(scheme, n, bits)


@pytest.mark.parametrize("narrow", [False, True])
@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (128, [60, 40, 40, 60])])
def test_flush_boundaries(emu, n, bits, narrow):
    import conv2d_scalars_cases as CV
    CV.case_flush(n, bits, narrow)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), MID])
def test_cuts(emu, n, bits):
    import conv2d_scalars_cases as CV
    CV.case_cuts("ckks", n, bits)


def test_natural_slices(emu):
    import conv2d_scalars_cases as CV
    CV.case_natural_slices("bgv", *MID)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (128, [60, 40, 40, 60])])
def test_every_built_tile_and_hint(emu, n, bits):
    """the per-lane and the wave-uniform path"""
    import conv2d_scalars_cases as CV
    CV.case_tiles(n, bits)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (128, [60, 40, 60])])
def test_untouched_neighbours(emu, n, bits):
    import conv2d_scalars_cases as CV
    CV.case_neighbours("bfv", n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_out_of_place(emu, scheme):
    import conv2d_scalars_cases as CV
    CV.case_out_of_place(scheme, *DEFERS)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_transparent_check(emu, scheme):
    import conv2d_scalars_cases as CV
    CV.case_transparent_check(scheme, *DEFERS)


def test_pending_state(emu):
    import conv2d_scalars_cases as CV
    CV.case_pending(*DEFERS)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_errors(emu, scheme):
    import conv2d_scalars_cases as CV
    CV.case_errors(scheme, *DEFERS)
