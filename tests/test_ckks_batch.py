"""CPU: batched CKKS encoding in device memory (CKKSEncoder_EncodeDevice / _DecodeDevice) with the kernels emulated, against
the REAL reference (oracle/_ref) where it is built.  Sizes up to 4096 take the one-launch transform, 8192 and 16384 the two-pass
split; the development build's SEALHIP_CKKS_FFT_BLOCK_LOG / SEALHIP_CKKS_SCRATCH_BYTES reach every column-stage count and the
chunk edges at small N."""
import pytest

import sealref

needs_ref = pytest.mark.skipif(not sealref.available(), reason="oracle/_ref (the real reference) is not built")

SIZES = [(8, [30, 30]), (1024, [40, 30, 40]), (4096, [60, 40, 40, 60]), (8192, [40, 40]), (16384, [50, 40, 50])]


@needs_ref
@pytest.mark.parametrize("n,bits", SIZES)
def test_encode_decode_parity(emu, n, bits):
    import ckks_batch_cases as CB
    CB.case_encode_decode_parity(n, bits, batch=3)


@needs_ref
def test_widths_mixed_in_one_batch(emu):
    """a chain above 180 bits: one batch holds 64-bit, 128-bit and multi-precision coefficients"""
    import ckks_batch_cases as CB
    widths = CB.case_encode_decode_parity(1024, [60, 50, 50, 50, 50, 60], batch=7, counts=(512,), levels=(4,))
    assert {64, 128, 0} <= widths, widths


@needs_ref
@pytest.mark.parametrize("block_log,scratch", [(9, None), (7, None), (6, 3 << 16), (5, 1 << 16)])
def test_pass_split_and_chunks(emu, monkeypatch, block_log, scratch):
    """N = 1024 cut at 2^block_log (1 .. 5 column stages); a small scratch cap makes chunks of a few items"""
    import ckks_batch_cases as CB
    monkeypatch.setenv("SEALHIP_CKKS_FFT_BLOCK_LOG", str(block_log))
    if scratch:
        monkeypatch.setenv("SEALHIP_CKKS_SCRATCH_BYTES", str(scratch))
    CB.case_encode_decode_parity(1024, [60, 50, 50, 60], batch=7, counts=(512, 5))
    CB.case_decode_random_words(1024, [40, 30, 40], batch=5)


@needs_ref
@pytest.mark.parametrize("n,bits", [(1024, [40, 30, 40]), (8192, [40, 40])])
def test_decode_random_words(emu, n, bits):
    import ckks_batch_cases as CB
    CB.case_decode_random_words(n, bits, batch=3)


@needs_ref
@pytest.mark.parametrize("n,bits", [(1024, [40, 30, 40]), (8192, [40, 40])])
def test_errors(emu, n, bits):
    import ckks_batch_cases as CB
    CB.case_errors(n, bits)


@needs_ref
def test_client_loop(emu):
    import ckks_batch_cases as CB
    CB.case_client_loop(1024, [60, 40, 40, 60], batch=3)


@needs_ref
@pytest.mark.parametrize("n,bits", [(1024, [60, 40, 60]), (8192, [60, 40, 60])])
def test_round_trip(emu, n, bits):
    import ckks_batch_cases as CB
    CB.case_round_trip(n, bits, batch=3)


@needs_ref
@pytest.mark.parametrize("n,bits", [(8, [30, 30]), (4096, [50, 40, 50]), (8192, [40, 40])])
def test_batch_of_one(emu, n, bits):
    import ckks_batch_cases as CB
    CB.case_batch_of_one(n, bits)
