"""CPU: one plaintext per item of a device-resident batch (Evaluator_AddPlainDevice / SubPlainDevice / MultiplyPlainDevice /
TransformPlainToNTTDevice) with the kernels emulated.  Against the REAL reference (oracle/_ref) where it is built, and against the
per-object forms on batches of one everywhere.  The development build's SEALHIP_PLAIN_SCRATCH_BYTES makes chunks of a few lifted
plaintexts at small N."""
import pytest

import sealref

needs_ref = pytest.mark.skipif(not sealref.available(), reason="oracle/_ref (the real reference) is not built")

SCHEMES = ["ckks", "bfv", "bgv"]
SIZES = [(8, [30, 30, 30]), (1024, [60, 40, 60]), (4096, [60, 40, 40, 60])]


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", SIZES)
def test_parity(emu, scheme, n, bits):
    import plain_batch_cases as PB
    PB.case_parity(scheme, n, bits, batch=3)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_batch_of_one(emu, scheme):
    import plain_batch_cases as PB
    PB.case_parity(scheme, 1024, [60, 40, 60], batch=1, sizes=(2,))


@pytest.mark.parametrize("scheme", SCHEMES)
def test_lowest_level(emu, scheme):
    """K = 1"""
    import plain_batch_cases as PB
    PB.case_parity(scheme, 1024, [60, 40, 60], batch=3, sizes=(2,), ci=0)


@pytest.mark.parametrize("scheme", ["bfv", "bgv"])
def test_branches_fast_lift(emu, scheme):
    """t (20 bits) below every prime of the level: the monomial items' words differ from the generic path's"""
    import plain_batch_cases as PB
    assert PB.case_branches(scheme, 1024, [60, 40, 60])


@pytest.mark.parametrize("scheme", ["bfv", "bgv"])
def test_branches_general_lift(emu, scheme):
    """t (40 bits) above the 30-bit primes of the level: the increment per prime.  The context builder accepts these parameters at
    N = 1024 (t only has to stay below the level's whole modulus, 60 bits here)."""
    import plain_batch_cases as PB
    assert not PB.case_branches(scheme, 1024, [30, 30, 60], tbits=40)


@needs_ref
@pytest.mark.parametrize("scheme", ["bfv", "bgv"])
@pytest.mark.parametrize("bits,tbits,fast", [([40, 40, 60], 20, True), ([30, 30, 60], 40, False)])
def test_shared_plaintext(emu, scheme, bits, tbits, fast):
    """one Plaintext of 1, 5, N - 1 and N coefficients for a batch of 3 at N = 64, two primes, against the reference item by item;
    t below every prime (fast plain lift) and above them (general lift)"""
    import plain_batch_cases as PB
    assert PB.case_shared_plaintext(scheme, 64, bits, tbits) == fast


@pytest.mark.parametrize("scheme", ["bfv", "bgv"])
def test_transform(emu, scheme):
    import plain_batch_cases as PB
    PB.case_transform(scheme, 1024, [60, 40, 40, 60], batch=3)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_out_of_place(emu, scheme):
    import plain_batch_cases as PB
    PB.case_out_of_place(scheme, 1024, [60, 40, 60])


@pytest.mark.parametrize("scheme", ["bfv", "bgv"])
@pytest.mark.parametrize("per_chunk", [1, 3])
def test_chunks(emu, monkeypatch, scheme, per_chunk):
    import plain_batch_cases as PB
    PB.case_chunks(scheme, 1024, [60, 40, 60], 7, per_chunk, monkeypatch)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_errors(emu, scheme):
    import plain_batch_cases as PB
    PB.case_errors(scheme, 1024, [60, 40, 60])


@pytest.mark.parametrize("scheme", SCHEMES)
def test_transparent_check(emu, scheme):
    import plain_batch_cases as PB
    PB.case_transparent_check(scheme, 1024, [60, 40, 60])


@needs_ref
def test_pipeline_ckks(emu):
    import plain_batch_cases as PB
    PB.case_pipeline_ckks(1024, [60, 40, 40, 60], batch=3)


@needs_ref
def test_pipeline_bfv(emu):
    import plain_batch_cases as PB
    PB.case_pipeline_bfv(1024, [60, 40, 60], batch=3)
