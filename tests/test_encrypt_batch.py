"""CPU: batched encryption in device memory (Encryptor_EncryptSymmetricDevice / Encryptor_EncryptDevice) with the kernels
emulated.  Against the REAL reference (oracle/_ref) where it is built, and against the per-object Encryptor forms everywhere.
N = 8 takes every per-item fallback (the ring is too small for the device's uniform sampler and 6 N bytes of noise are no whole
64-byte pieces); the development build's SEALHIP_ENCRYPT_SCRATCH_BYTES makes chunks of a few items at small N."""
import pytest

import sealref

needs_ref = pytest.mark.skipif(not sealref.available(), reason="oracle/_ref (the real reference) is not built")

SCHEMES = ["ckks", "bfv", "bgv"]
SIZES = [(8, [30, 30, 30]), (1024, [60, 40, 60]), (4096, [60, 40, 40, 60]), (8192, [60, 60])]


@needs_ref
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", SIZES)
def test_reference_parity(emu, scheme, n, bits):
    import encrypt_batch_cases as EB
    EB.case_reference_parity(scheme, n, bits, batch=3)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", SIZES)
def test_per_item_seeds(emu, scheme, n, bits):
    import encrypt_batch_cases as EB
    EB.case_per_item_seeds(scheme, n, bits, batch=3)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_batch_of_one(emu, scheme):
    import encrypt_batch_cases as EB
    EB.case_per_item_seeds(scheme, 1024, [60, 40, 60], batch=1)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", [(1024, [60, 40, 60]), (8192, [60, 60])])
def test_fresh_entropy(emu, scheme, n, bits):
    import encrypt_batch_cases as EB
    EB.case_fresh_entropy(scheme, n, bits, batch=4)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", [(1024, [60, 40, 60]), (4096, [60, 60])])
def test_host_sampling_equals_device(emu, monkeypatch, scheme, n, bits):
    import encrypt_batch_cases as EB
    EB.case_host_sampling_equals_device(scheme, n, bits, 3, monkeypatch)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("per_chunk", [1, 3])
def test_chunks(emu, monkeypatch, scheme, per_chunk):
    import encrypt_batch_cases as EB
    EB.case_chunks(scheme, 1024, [60, 40, 60], 7, per_chunk, monkeypatch)


@needs_ref
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("per_chunk", [1, 3])
def test_chunks_against_reference(emu, monkeypatch, scheme, per_chunk):
    import encrypt_batch_cases as EB
    EB.case_chunks(scheme, 1024, [60, 40, 60], 7, per_chunk, monkeypatch, with_ref=True)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_errors(emu, scheme):
    import encrypt_batch_cases as EB
    EB.case_errors(scheme, 1024, [60, 40, 60])


@needs_ref
def test_pipeline(emu):
    import encrypt_batch_cases as EB
    EB.case_pipeline(1024, [60, 40, 40, 60], batch=3)
