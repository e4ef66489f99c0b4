"""CPU (emulated kernels): the C layer outside Evaluator_* - which NULL every export of capi_core.cpp, capi_containers.cpp and
capi_client.cpp answers with E_POINTER, what the six *_Save exports answer for every capacity and compression mode, the order in
which the context-taking loads refuse, and the SecretKey / PublicKey copies (tests/capi_object_cases.py holds the cases and the
tables recorded before these entries were folded)."""
import ctypes as C

import pytest

import seal_amd._native as N
import capi_object_cases as cases
import sealref
import test_cabi
import test_host_paths

n = 64
E_POINTER = N.E_POINTER

# ---- every export of the three files, one word per argument.  Capitals: a NULL there is E_POINTER.  Lower case: never E_POINTER -
#      a value (u64, dbl, ...), an ignored handle (pool, stream), or a pointer that is optional or that the C++ layer refuses as
#      an invalid argument (ptr, bytes, dev, pid, seed, list, pk, sk).  THIS is an object of the kind the symbol's prefix names.
LOAD, SAVE, SIZE = "THIS CTX BYTES u64 OUT", "THIS BYTES u64 u8 OUT", "THIS u8 OUT"
EXPORTS = {
    "SealHip_Version": "OUT OUT OUT", "SealHip_DeviceInfo": "bytes u64 ptr ptr", "SealHip_LastError": "bytes OUT",
    "CoeffModulus_Create1": "u64 u64 OUT OUT", "PlainModulus_Batching": "u64 int OUT", "EncParams_Create1": "u8 OUTH",
    "EncParams_Destroy": "THIS", "EncParams_SetPolyModulusDegree": "THIS u64", "EncParams_GetPolyModulusDegree": "THIS OUT",
    "EncParams_SetCoeffModulus": "THIS u64 OUT", "EncParams_GetCoeffModulus": "THIS OUT ptr",
    "EncParams_SetPlainModulus2": "THIS u64", "EncParams_GetScheme": "THIS OUT", "SEALContext_Create": "PARMS bool int OUTH",
    "SEALContext_Destroy": "THIS", "SEALContext_KeyParmsId": "THIS PID", "SEALContext_FirstParmsId": "THIS PID",
    "SEALContext_LastParmsId": "THIS PID", "SEALContext_UsingKeyswitching": "THIS OUT", "SEALContext_ChainIndex": "THIS PID OUT",
    "SEALContext_ParmsIdAt": "THIS u64 PID", "SEALContext_CoeffModulusAt": "THIS u64 OUT ptr",
    "SEALContext_TotalCoeffModulusBitCount": "THIS u64 OUT", "SEALContext_SetParmsId": "THIS u64 PID",
    "SEALContext_NTTRoot": "THIS u64 OUT", "SEALContext_BaseBsk": "THIS u64 OUT ptr", "Ciphertext_Create3": "CTX pool OUTH",
    "Ciphertext_CreateBatch": "CTX u64 OUTH", "Ciphertext_Create2": "THIS OUTH", "Ciphertext_Set": "THIS THIS",
    "Ciphertext_Destroy": "THIS", "Ciphertext_Resize1": "THIS CTX PID u64", "Ciphertext_ParmsId": "THIS PID",
    "Ciphertext_SetIsNTTForm": "THIS bool", "Ciphertext_SetScale": "THIS dbl", "Ciphertext_SetCorrectionFactor": "THIS u64",
    "Ciphertext_IsTransparent": "THIS OUT", "Ciphertext_DevicePtr": "THIS OUT ptr", "Ciphertext_CopyFromHost": "THIS OUT u64",
    "Ciphertext_CopyToHost": "THIS OUT u64", "Ciphertext_CopyWordsToHost": "THIS u64 u64 OUT",
    "Ciphertext_CopyFromDevice": "THIS DEV u64 stream", "Ciphertext_Load": LOAD, "Ciphertext_UnsafeLoad": LOAD,
    "Ciphertext_LoadItem": "THIS CTX u64 BYTES u64 OUT", "Ciphertext_SaveSize": SIZE,
    "Ciphertext_SaveItem": "THIS u64 BYTES u64 u8 OUT", "Ciphertext_Save": SAVE, "Plaintext_Load": LOAD,
    "Plaintext_UnsafeLoad": LOAD, "Plaintext_SaveSize": SIZE, "Plaintext_Save": SAVE, "KSwitchKeys_SaveSize": SIZE,
    "KSwitchKeys_Save": SAVE, "KSwitchKeys_DeviceBytes": "THIS OUT", "KSwitchKeys_Load": LOAD, "KSwitchKeys_UnsafeLoad": LOAD,
    "Plaintext_Create1": "CTX OUTH", "Plaintext_Create5": "THIS OUTH", "Plaintext_Destroy": "THIS",
    "Plaintext_Set4": "THIS u64 OUT", "Plaintext_SetFromDevice": "THIS u64 DEV",      # (the pointer is looked at when the count is not 0)
    "Plaintext_CoeffCount": "THIS OUT", "Plaintext_IsNTTForm": "THIS OUT", "Plaintext_GetParmsId": "THIS PID",
    "Plaintext_SetParmsId": "THIS PID", "Plaintext_Scale": "THIS OUT", "Plaintext_SetScale": "THIS dbl",
    "Plaintext_CopyToHost": "THIS OUT u64", "Ciphertext_Size": "THIS OUT", "Ciphertext_BatchCount": "THIS OUT",
    "Ciphertext_PolyModulusDegree": "THIS OUT", "Ciphertext_CoeffModulusSize": "THIS OUT", "Ciphertext_IsNTTForm": "THIS OUT",
    "Ciphertext_Scale": "THIS OUT", "Ciphertext_CorrectionFactor": "THIS OUT", "Ciphertext_Create4": "CTX PID pool OUTH",
    "Ciphertext_Create5": "CTX PID u64 pool OUTH", "Ciphertext_Reserve1": "THIS CTX PID u64",
    "Ciphertext_Reserve2": "THIS CTX u64", "Ciphertext_Reserve3": "THIS u64", "Ciphertext_SizeCapacity": "THIS OUT",
    "Ciphertext_SetParmsId": "THIS PID", "Ciphertext_Resize2": "THIS CTX u64", "Ciphertext_Resize3": "THIS u64",
    "Ciphertext_Resize4": "THIS u64 u64 u64", "Ciphertext_GetDataAt1": "THIS u64 OUT", "Ciphertext_GetDataAt2": "THIS u64 u64 OUT",
    "Ciphertext_SetDataAt": "THIS u64 u64", "Ciphertext_Release": "THIS", "KSwitchKeys_Create2": "THIS OUTH",
    "KSwitchKeys_Set": "THIS THIS", "KSwitchKeys_RawSize": "THIS OUT", "KSwitchKeys_GetKeyList": "THIS u64 OUT list",
    "KSwitchKeys_ClearDataAndReserve": "THIS u64", "KSwitchKeys_AddKeyList": "THIS u64 LIST", "KSwitchKeys_GetParmsId": "THIS PID",
    "KSwitchKeys_SetParmsId": "THIS PID", "SEALContext_ParametersSet": "THIS OUT",
    "SEALContext_ParameterErrorName": "THIS bytes OUT", "SEALContext_ParameterErrorMessage": "THIS bytes OUT",
    "SEALContext_KeyContextData": "THIS OUTH", "SEALContext_FirstContextData": "THIS OUTH",
    "SEALContext_LastContextData": "THIS OUTH", "SEALContext_GetContextData": "THIS PID OUTH", "ContextData_Destroy": "THIS",
    "ContextData_TotalCoeffModulus": "THIS OUT ptr", "ContextData_TotalCoeffModulusBitCount": "THIS OUT",
    "ContextData_Parms": "THIS OUTH", "ContextData_Qualifiers": "THIS OUTH", "ContextData_CoeffDivPlainModulus": "THIS OUT ptr",
    "ContextData_PlainUpperHalfThreshold": "THIS OUT", "ContextData_PlainUpperHalfIncrement": "THIS OUT ptr",
    "ContextData_UpperHalfThreshold": "THIS OUT ptr", "ContextData_UpperHalfIncrement": "THIS OUT ptr",
    "ContextData_PrevContextData": "THIS OUTH", "ContextData_NextContextData": "THIS OUTH", "ContextData_ChainIndex": "THIS OUT",
    "ContextData_ParmsId": "THIS PID", "EPQ_Destroy": "THIS", "EncParams_Create2": "THIS OUTH", "EncParams_Set": "THIS THIS",
    "EncParams_GetParmsId": "THIS PID", "EncParams_GetPlainModulus": "THIS OUT", "EncParams_Equals": "THIS THIS OUT",
    "EncParams_SaveSize": SIZE, "EncParams_Save": SAVE, "EncParams_Load": "THIS BYTES u64 OUT",
    "SecretKey_Create2": "THIS OUTH", "SecretKey_Assign": "THIS THIS", "SecretKey_ParmsId": "THIS PID",
    "SecretKey_SaveSize": SIZE, "SecretKey_Save": SAVE, "PublicKey_Create2": "THIS OUTH",
    "PublicKey_Assign": "THIS THIS", "PublicKey_ParmsId": "THIS PID", "PublicKey_SaveSize": SIZE,
    "PublicKey_Save": SAVE, "EPQ_ParametersSet": "THIS OUT", "EPQ_UsingFFT": "THIS OUT",
    "EPQ_UsingNTT": "THIS OUT", "EPQ_UsingBatching": "THIS OUT", "EPQ_UsingFastPlainLift": "THIS OUT",
    "EPQ_UsingDescendingModulusChain": "THIS OUT", "EPQ_SecLevel": "THIS OUT", "SecretKey_Create": "CTX OUTH",
    "SecretKey_Destroy": "THIS", "KeyGenerator_Create1": "CTX seed OUTH", "KeyGenerator_Create2": "CTX SK seed OUTH",
    "KeyGenerator_Destroy": "THIS", "KeyGenerator_SecretKey": "THIS SK", "KeyGenerator_CreatePublicKey": "THIS PK",
    "KeyGenerator_CreateRelinKeys": "THIS KSK", "KeyGenerator_CreateGaloisKeysFromElts": "THIS u64 ptr KSK",
    "KeyGenerator_CreateGaloisKeysFromSteps": "THIS u64 ptr KSK", "KeyGenerator_CreateGaloisKeysAll": "THIS KSK",
    "KeyGenerator_SeededSaveSize": "THIS bool u64 OUT", "KeyGenerator_CreateRelinKeysSave": "THIS BYTES u64 OUT",
    "KeyGenerator_CreateGaloisKeysFromEltsSave": "THIS u64 ptr BYTES u64 OUT", "KeyGenerator_KeyToHost": "THIS u32 OUT u64",
    "SecretKey_Get": "THIS OUT", "PublicKey_Get": "THIS OUT", "SecretKey_Set": "THIS OUT u64",
    "SecretKey_Load": LOAD, "SecretKey_UnsafeLoad": LOAD,
    "Decryptor_Create": "CTX SK OUTH", "Decryptor_Destroy": "THIS", "Decryptor_Decrypt": "THIS CT PT",
    "Decryptor_InvariantNoiseBudget": "THIS CT OUT", "Decryptor_DecryptBatchWords": "THIS CT OUT",
    "Decryptor_DecryptBatch": "THIS CT DEV u64", "CKKSEncoder_Create": "CTX OUTH", "CKKSEncoder_Destroy": "THIS",
    "CKKSEncoder_SlotCount": "THIS OUT", "CKKSEncoder_Encode1": "THIS u64 ptr PID dbl PT pool",
    "CKKSEncoder_Encode2": "THIS u64 ptr PID dbl PT pool", "CKKSEncoder_Encode3": "THIS dbl PID dbl PT pool",
    "CKKSEncoder_Encode4": "THIS dbl dbl PID dbl PT pool", "CKKSEncoder_Encode5": "THIS i64 PID PT",
    "CKKSEncoder_Decode1": "THIS PT OUT ptr pool", "CKKSEncoder_Decode2": "THIS PT OUT ptr pool",
    "CKKSEncoder_EncodeDevice": "THIS dev u64 u64 bool pid dbl dev", "CKKSEncoder_EncodeScalars": "THIS u64 ptr pid dbl dev",
    "CKKSEncoder_EncodeIntegerScalars": "THIS u64 ptr pid dev", "CKKSEncoder_DecodeDevice": "THIS dev u64 pid dbl bool dev",
    "BatchEncoder_Create": "CTX OUTH", "BatchEncoder_Destroy": "THIS", "BatchEncoder_GetSlotCount": "THIS OUT",
    "BatchEncoder_Encode1": "THIS u64 ptr PT", "BatchEncoder_Encode2": "THIS u64 ptr PT",
    "BatchEncoder_Decode1": "THIS PT OUT OUT pool", "BatchEncoder_Decode2": "THIS PT OUT OUT pool",
    "BatchEncoder_EncodeDevice": "THIS dev u64 bool dev", "BatchEncoder_DecodeDevice": "THIS dev u64 bool dev",
    "PublicKey_Create": "CTX OUTH", "PublicKey_Destroy": "THIS", "PublicKey_Set": "THIS OUT u64",
    "PublicKey_Load": LOAD, "PublicKey_UnsafeLoad": LOAD,
    "Encryptor_Create": "CTX pk sk OUTH", "Encryptor_Encrypt": "THIS PT CT pool", "Encryptor_EncryptZero1": "THIS PID CT pool",
    "Encryptor_EncryptZero2": "THIS CT pool", "Encryptor_EncryptZeroSymmetric2": "THIS bool CT pool", "Encryptor_Destroy": "THIS",
    "Encryptor_SetSeed": "THIS seed", "Encryptor_EncryptZeroSymmetric1": "THIS PID bool CT pool",
    "Encryptor_EncryptSymmetric": "THIS PT bool CT pool", "Encryptor_SymmetricSaveSize": "THIS PID OUT",
    "Encryptor_EncryptZeroSymmetricSave": "THIS PID BYTES u64 OUT", "Encryptor_EncryptSymmetricSave": "THIS PT BYTES u64 OUT",
    "Encryptor_EncryptSymmetricDevice": "THIS dev u64 pid dbl seed CT", "Encryptor_EncryptDevice": "THIS dev u64 pid dbl seed CT",
}
# the rest of include/sealhip.h: capi_kernels.cpp (raw kernel seams, communicator, item maps, key upload) and diagnostics.cpp
ELSEWHERE = """
Comm_AllReduceWords Comm_BroadcastWords Comm_Create Comm_Destroy Comm_DigitRange Comm_GetUniqueId Comm_Info Comm_RcclAvailable
GaloisKeys_GetIndex GaloisTool_GetEltFromStep Graph_Destroy ItemMap_Create ItemMap_Destroy ItemMap_Info KSwitchKeys_Create1
KSwitchKeys_Destroy KSwitchKeys_HasKey KSwitchKeys_SetKey KSwitchKeys_SetKeyDigits KSwitchKeys_SetKeyFromDevice KSwitchKeys_Size
RelinKeys_GetIndex SealHip_GaloisStats SealHip_InstallAbortTrace SealHip_KsChunkStats SealHip_PoolStats SealHip_ProductStats
SealHip_ReleasePool SealHip_SetStagedHostCopies SealHip_TailStats SealHip_XofStats shl_apply_galois shl_conv2d_scalars
shl_conv2d_scalars_tile shl_device_count shl_device_synchronize shl_dot_items shl_dot_items_flush_interval shl_dot_scalars
shl_dot_scalars_info shl_dot_scalars_mapped shl_dot_scalars_mapped_info shl_dot_scalars_tile shl_dyadic_product shl_free
shl_malloc shl_matmul_items shl_matmul_items_info shl_matmul_items_tile shl_matmul_plain_items shl_matmul_plain_items_info
shl_matmul_plain_items_tile shl_matmul_scalars shl_matmul_scalars_info shl_matmul_scalars_tile shl_memcpy_d2h shl_memcpy_h2d
shl_ntt_forward shl_ntt_inverse shl_reduce_flush_intervals shl_reduce_items shl_reduce_mapped shl_rns_stage shl_set_device
shl_stream_create shl_stream_destroy shl_timer_create shl_timer_destroy shl_timer_start shl_timer_stop
""".split()


@pytest.fixture(scope="module")
def objects(emu):
    return cases.Objects(emu, n, [40, 30, 30, 40], 21)


@pytest.fixture(scope="module")
def arguments(objects):
    """a valid argument of every kind (live objects of one CKKS context), kept alive beside the ctypes values"""
    S, d, L = objects.S, objects.d, N.lib()
    dest, plain2 = S.Ciphertext(d.ctx), S.Plaintext(d.ctx)
    level, epq = d.ctx.key_context_data(), C.c_void_p()
    N.check(L.ContextData_Qualifiers(level._h, C.byref(epq)))
    decryptor, encoder = S.Decryptor(d.ctx, objects.sk), S.CKKSEncoder(d.ctx)
    encryptor = S.Encryptor(d.ctx, secret_key=objects.sk)
    words = S.DeviceBuffer(4 * (objects.K + 1) * n)
    host = (C.c_uint64 * (1 << 16))()              # room for whatever an entry could write through an OUT or BYTES argument
    not_a_batch_encoder = (C.c_uint64 * 64)()      # (a CKKS context has none; a call with a NULL elsewhere returns before it looks)
    keep = [dest, plain2, level, decryptor, encoder, encryptor, words, host, not_a_batch_encoder]
    this = {"Ciphertext": objects.ct._h, "Plaintext": objects.pt._h, "KSwitchKeys": objects.ksk._h, "SEALContext": d.ctx._h,
            "ContextData": level._h, "EPQ": epq, "EncParams": d.parms._h, "SecretKey": objects.sk._h, "PublicKey": objects.pk._h,
            "KeyGenerator": objects.kg._h, "Decryptor": decryptor._h, "CKKSEncoder": encoder._h, "Encryptor": encryptor._h,
            "BatchEncoder": C.c_void_p(C.addressof(not_a_batch_encoder))}
    values = {
        "CTX": d.ctx._h, "PARMS": d.parms._h, "CT": dest._h, "PT": plain2._h, "KSK": objects.ksk._h, "SK": objects.sk._h,
        "PK": objects.pk._h, "PID": (C.c_uint64 * 4)(*objects.pid), "OUT": host, "BYTES": host, "OUTH": C.pointer(C.c_void_p()),
        "DEV": C.c_void_p(words.ptr), "LIST": (C.c_void_p * 2)(objects.pk._h.value, objects.pk._h.value),
        "dev": C.c_void_p(words.ptr), "ptr": host, "bytes": host, "pid": (C.c_uint64 * 4)(*objects.pid), "seed": host, "list": host,
        "pk": objects.pk._h, "sk": objects.sk._h, "pool": None, "stream": None, "u64": C.c_uint64(1), "u32": C.c_uint32(3),
        "u8": C.c_uint8(0), "int": C.c_int(1), "i64": C.c_int64(1), "dbl": C.c_double(2.0 ** 20), "bool": C.c_bool(False),
    }
    yield values, this, keep
    N.check(L.EPQ_Destroy(epq))


def test_every_declared_symbol_is_in_a_table():
    declared = test_cabi.declared_symbols()
    tables = sorted(list(EXPORTS) + list(test_host_paths.EXPORTS) + ELSEWHERE)
    assert tables == declared, sorted(set(tables) ^ set(declared))
    assert declared == sorted(N.SYMBOLS)


@pytest.mark.parametrize("symbol", sorted(EXPORTS))
def test_null_in_a_checked_position_is_e_pointer(arguments, symbol):
    values, this, _ = arguments
    kinds = EXPORTS[symbol].split()
    checked = [i for i, k in enumerate(kinds) if k.isupper()]
    fn = getattr(N.lib(), symbol)
    for i in checked:
        args = [None if j == i else this[symbol.split("_")[0]] if k == "THIS" else values[k] for j, k in enumerate(kinds)]
        assert fn(*args) & 0xFFFFFFFF == E_POINTER, (symbol, "argument %d (%s)" % (i, kinds[i]))


def test_unchecked_pointers_are_never_e_pointer(arguments, objects):
    """the pointers in lower case that a call survives as NULL: optional outputs, and pointers the C++ layer refuses itself"""
    values, this, _ = arguments
    S, d, L = objects.S, objects.d, N.lib()
    calls = {   # symbol -> the positions given as NULL (one call each, the others valid)
        "KSwitchKeys_GetKeyList": [3], "Ciphertext_DevicePtr": [2], "Encryptor_SetSeed": [1], "Encryptor_Create": [1, 2],
        "EncParams_GetCoeffModulus": [2], "SEALContext_CoeffModulusAt": [3], "SEALContext_BaseBsk": [3],
        "SEALContext_ParameterErrorName": [1], "SEALContext_ParameterErrorMessage": [1], "ContextData_TotalCoeffModulus": [2],
        "ContextData_PlainUpperHalfIncrement": [2], "ContextData_UpperHalfThreshold": [2], "SealHip_LastError": [0],
        "SealHip_DeviceInfo": [0, 2, 3], "KeyGenerator_Create1": [1],
        "CKKSEncoder_EncodeDevice": [1, 5, 7], "CKKSEncoder_EncodeScalars": [2, 3, 5], "CKKSEncoder_EncodeIntegerScalars": [2, 3, 4],
        "CKKSEncoder_DecodeDevice": [1, 3, 6], "Encryptor_EncryptSymmetricDevice": [1, 3], "Encryptor_EncryptDevice": [1, 3],
    }
    for symbol, positions in calls.items():
        kinds, prefix = EXPORTS[symbol].split(), symbol.split("_")[0]
        for i in positions:
            assert not kinds[i].isupper(), (symbol, i)
            made = C.c_void_p()
            args = [None if j == i else this[prefix] if k == "THIS" else C.byref(made) if k == "OUTH" else values[k]
                    for j, k in enumerate(kinds)]
            assert getattr(L, symbol)(*args) & 0xFFFFFFFF != E_POINTER, (symbol, "argument %d (%s)" % (i, kinds[i]))
            if made.value:
                N.check(getattr(L, prefix + "_Destroy")(made))
    assert cases.outcome(L.Encryptor_Create(d.ctx._h, None, None, C.byref(C.c_void_p()))) == \
        (N.E_INVALIDARG, "neither a public key nor a secret key is set")


def test_save_matrix(objects):
    """six objects x capacities 8, 16, 64, cap - 1, cap x modes none, zlib, zstd, unknown: HRESULT and words of every cell"""
    rows = cases.save_matrix(objects)
    assert len(rows) >= 6 * (2 * 5 + 5 + 1)
    assert [r for r in rows if r[3] != r[4]] == []


@pytest.mark.skipif(not sealref.available(), reason="oracle/_ref (the real reference) is not built")
def test_encryption_parameters_save_refuses_as_the_reference(objects):
    """EncryptionParameters::save of the reference into a buffer of the caller's size (serialization.cpp:193, 548: "insufficient
    size" below a header; :36-54: the put buffer overflows above it) against EncParams_Save, uncompressed, at every capacity of the
    matrix.  The cell at 8 bytes was COR_E_IO before EncParams_Save went through the shared save path."""
    import ctypes as C
    ref = sealref.RefContext("ckks", n, objects.primes, 0)
    key = len(objects.primes) - 1                    # the chain index of the key level, what objects.d.parms holds
    whole = ref.parms_save(key)
    assert whole == cases.stream("EncParams", objects.d.parms)
    classes = {1: N.E_INVALIDARG, 4: N.COR_E_IO, 0: 0}   # the shim's codes: std::invalid_argument, any other exception, none
    for capacity in (8, 16, 64, len(whole) - 1, len(whole)):
        buf, nb = (C.c_uint8 * capacity)(), C.c_uint64()
        rc = sealref.lib().ref_parms_save(ref.h, C.c_uint64(key), C.c_int(0), buf, C.c_uint64(capacity), C.byref(nb))
        assert cases.save("EncParams", objects.d.parms, capacity, 0)[0][0] == classes[rc], capacity


def test_save_special_cases(objects):
    assert cases.mismatches(cases.save_special_cases(objects), cases.SAVE_SPECIAL) == []


def test_load_order_of_refusals(objects):
    assert cases.mismatches(cases.load_order(objects), cases.LOAD_ORDER) == []


def test_key_object_copies(objects):
    assert cases.mismatches(cases.key_copies(objects), cases.KEY_COPIES) == []
