"""`-m gpu`: the reference's wire format on the real device path — streams written by the REAL reference
(oracle/_ref) are parsed into the HBM slabs through the C ABI; loaded words, re-saved bytes, key-switching results with keys
loaded from (seeded) streams and exception classes must equal the reference's.  Includes the headline size (N = 2^16, L = 16:
a 126 MB seeded relinearization key expanded with the Blake2xb PRNG restated in seal_amd/csrc/blake2.h)."""
import pytest

import sealref
import serial_cases as SC

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not sealref.available(), reason="oracle/_ref (the real reference) did not travel")]

SIZES = [("ckks", 8192, [60, 40, 40, 60]), ("bfv", 4096, [36, 36, 37]), ("bgv", 8192, [50, 40, 56])]


@pytest.mark.parametrize("scheme,n,bits", SIZES)
def test_parms_ids_and_ciphertext_streams(gpu, scheme, n, bits):
    SC.case_parms_ids(scheme, n, bits)
    SC.case_ciphertext_streams(scheme, n, bits)
    SC.case_evaluated_ciphertext_roundtrip(scheme, n, bits)


def test_bgv_coefficient_form_stream(gpu):
    SC.case_bgv_coefficient_form_stream(8192, [50, 40, 56])


def test_batch_items(gpu):
    SC.case_batch_items("ckks", 8192, [60, 40, 40, 60])


@pytest.mark.parametrize("scheme,n,bits,seeded", [
    ("ckks", 8192, [60, 40, 40, 60], True), ("ckks", 16384, [60, 50, 50, 60], False), ("bfv", 8192, [50, 55, 56], True),
    ("bgv", 4096, [36, 36, 37], True),
])
def test_key_streams(gpu, scheme, n, bits, seeded):
    SC.case_key_streams(scheme, n, bits, seeded)


@pytest.mark.parametrize("scheme,n,bits", [("ckks", 8192, [60, 40, 40, 60]), ("bfv", 8192, [50, 55, 56]), ("ckks", 32768, [60, 50, 50, 60])])
def test_key_save(gpu, scheme, n, bits):
    SC.case_key_save(scheme, n, bits)


def test_key_words_survive_save(gpu):
    SC.case_key_words_survive_save()


def test_key_stream_headline_size(gpu):
    """BASELINE's headline parameters: CKKS N = 65536, {60, 14 x 50, 60}; seeded RelinKeys + GaloisKeys streams"""
    SC.case_key_streams("ckks", 65536, [60] + [50] * 14 + [60], True)


def test_malformed_streams(gpu):
    SC.case_malformed_streams("ckks", 4096, [40, 30, 40])
    SC.case_malformed_key_streams("ckks", 4096, [40, 30, 40])


@pytest.mark.parametrize("scheme,n,bits", SIZES)
def test_plaintext_streams(gpu, scheme, n, bits):
    SC.case_plaintext_streams(scheme, n, bits)


# ---- decryption on the device
@pytest.mark.parametrize("scheme,n,bits", SIZES + [("ckks", 32768, [60, 50, 50, 50, 60])])
def test_decrypt(gpu, scheme, n, bits):
    import decrypt_cases as DC
    DC.case_decrypt(scheme, n, bits)


@pytest.mark.parametrize("scheme,n,bits", SIZES)
def test_end_to_end_streams(gpu, scheme, n, bits):
    import decrypt_cases as DC
    DC.case_end_to_end_streams(scheme, n, bits)


@pytest.mark.parametrize("scheme,n,bits", SIZES + [("ckks", 65536, [60] + [50] * 14 + [60])])
def test_encrypt_symmetric(gpu, scheme, n, bits):
    import decrypt_cases as DC
    DC.case_encrypt_symmetric(scheme, n, bits)


@pytest.mark.parametrize("scheme,n,bits", [("bfv", 4096, [36, 36, 37]), ("bgv", 8192, [50, 40, 56]), ("bfv", 32768, [55, 55, 55, 55])])
def test_batch_encoder(gpu, scheme, n, bits):
    import decrypt_cases as DC
    DC.case_batch_encoder(scheme, n, bits)


@pytest.mark.parametrize("scheme,n,bits", [("bfv", 8192, [50, 50, 50, 58]), ("bgv", 16384, [50, 50, 50, 50, 60])])
def test_slot_semantics(gpu, scheme, n, bits):
    import decrypt_cases as DC
    DC.case_slot_semantics(scheme, n, bits)


@pytest.mark.parametrize("scheme,n,bits", SIZES[:2] + [("ckks", 32768, [60, 50, 50, 60])])
def test_compressed_streams(gpu, scheme, n, bits):
    SC.case_compressed_streams(scheme, n, bits)


@pytest.mark.parametrize("scheme,n,bits", SIZES + [("ckks", 32768, [60, 50, 50, 50, 60])])
def test_encrypt_asymmetric(gpu, scheme, n, bits):
    import decrypt_cases as DC
    DC.case_encrypt_asymmetric(scheme, n, bits)


THRESHOLDS = [2, 8, 32, 1024]   # test_serialization.py: the ring sizes at which the Encryptor changes samplers


@pytest.mark.parametrize("scheme", ["ckks", "bfv", "bgv"])
@pytest.mark.parametrize("n", THRESHOLDS)
def test_encrypt_at_sampling_thresholds(gpu, scheme, n):
    import decrypt_cases as DC
    DC.case_encrypt_symmetric(scheme, n, [30, 30, 30])
    DC.case_encrypt_asymmetric(scheme, n, [30, 30, 30])


@pytest.mark.parametrize("scheme", ["ckks", "bfv", "bgv"])
@pytest.mark.parametrize("n", THRESHOLDS[1:])   # 8 is the smallest ring on which case_keygen's rotation by two steps exists
def test_keygen_at_sampling_thresholds(gpu, scheme, n):
    import decrypt_cases as DC
    DC.case_keygen(scheme, n, [30, 30, 30])


@pytest.mark.parametrize("n,bits", [(8192, [60, 40, 40, 60]), (32768, [60, 50, 50, 50, 60]), (65536, [60] + [50] * 14 + [60])])   # the last two reach the multi-precision branch (scale 2^150)
def test_ckks_encoder(gpu, n, bits):
    import decrypt_cases as DC
    DC.case_ckks_encoder(n, bits)


def test_example_ckks_basics(gpu):
    """native/examples/5_ckks_basics.cpp with its own parameters (N = 8192, {60, 40, 40, 60}, scale 2^40)"""
    import example_cases as EC
    EC.example_ckks_basics()


def test_example_batching_rotation(gpu):
    import example_cases as EC
    EC.example_batching_rotation()


@pytest.mark.parametrize("scheme,n,bits", [("ckks", 8192, [60, 40, 40, 60]), ("bfv", 16384, [50, 50, 50, 58]), ("bgv", 4096, [36, 36, 37]),
                                           ("ckks", 65536, [60] + [50] * 14 + [60])])
def test_keygen(gpu, scheme, n, bits):
    import decrypt_cases as DC
    DC.case_keygen(scheme, n, bits, elts=(3,) if n == 65536 else (3, 5))


@pytest.mark.parametrize("scheme,n,bits", [("ckks", 1024, [40, 30, 30, 40]), ("bfv", 8192, [50, 55, 56]), ("ckks", 8192, [60, 59, 60]),
                                           ("ckks", 65536, [60] + [50] * 14 + [60])])
def test_shake256_seeded_streams(gpu, scheme, n, bits):
    """the device SHAKE256 expansion (one thread per 4096-byte PRNG buffer), incl. primes with hundreds of redrawn words"""
    SC.case_shake256_seeded_streams(scheme, n, bits)


def test_object_save_matrix_and_load_order(gpu):
    """the C layer's pinned answers (tests/capi_object_cases.py) on the device, CKKS N = 4096 {40, 30, 40}: every cell of the save
    matrix, the special cases of the saves, the order of refusals of the loads, the key copies"""
    import capi_object_cases as cases
    objects = cases.Objects(gpu, 4096, [40, 30, 40], 22)
    assert [r for r in cases.save_matrix(objects) if r[3] != r[4]] == []
    assert cases.mismatches(cases.save_special_cases(objects), cases.SAVE_SPECIAL) == []
    assert cases.mismatches(cases.load_order(objects), cases.LOAD_ORDER) == []
    assert cases.mismatches(cases.key_copies(objects), cases.KEY_COPIES) == []
